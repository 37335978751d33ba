// slg_host.hpp — what the host translation units of the C ABI share (slg_index.hip, slg_batch.hip,
// slg_shard.hip, slg_rerank.hip, slg_vsearch.hip, slg_hybrid.hip, slg_aggs.hip, slg_rescore.hip, slg_bool.hip, slg_booltree.hip, slg_phrase.hip, slg_fscore.hip, slg_script.hip, slg_scan.hip, slg_collapse.hip, slg_tophits.hip, slg_composite.hip, slg_termbuckets.hip, slg_highlight.hip, slg_explain.hip): the error plumbing, device memory, the host
// structures behind the opaque handles and the small helpers several entry points use.  Private: not
// installed, not part of include/.  No kernel header is included here — each unit includes the one
// whose kernels it launches (slg_stage.hpp, slg_kernels.hpp, slg_rerank.hpp, slg_vsearch.hpp, slg_hybrid.hpp; the shard
// unit none), so every kernel is compiled once.
//
// Everything in namespace slghost has hidden visibility: shared between the library's objects, never
// part of its export list.
#pragma once

#include "../../include/searchlite_gpu.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "slg_desc.hpp"
#include "slg_expand_merge.hpp"
#include "slg_plan.hpp"

namespace slghost __attribute__((visibility("hidden"))) {

// the thread's last error (slg_last_error / slg_last_error_code): one thread-local object, in slg_index.hip
struct LastError {
  std::string msg;
  int code = SLG_OK;
};
LastError &last_error();

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

#define SLG_REQUIRE_LIVE(b) \
  SLG_REQUIRE((b) != nullptr && (b)->idx != nullptr, "batch is NULL or its index was destroyed")

template <typename F>
int guarded(F &&f) {
  LastError &le = last_error();
  auto fail = [&le](int code, const char *msg) {
    le.msg = msg;
    le.code = code;
  };
  try {
    le.msg.clear();
    le.code = SLG_OK;
    f();
  } catch (const SlgError &e) {
    fail(e.code, e.what());
  } catch (const std::bad_alloc &) {
    fail(SLG_ERR_OOM, "host allocation failed");
  } catch (const std::exception &e) {
    fail(SLG_ERR_INTERNAL, e.what());
  } catch (...) {
    fail(SLG_ERR_INTERNAL, "unknown error");
  }
  return le.code;
}

// Keeps the thread's last error across the clean-up that follows a failure (destroying a batch, an index
// or a group may reset it): the error at the guard's construction is the last error again when it goes
struct KeepLastError {
  const LastError kept = last_error();
  ~KeepLastError() { last_error() = kept; }
};

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

// a pinned staging image of at least n bytes: taken from the pool for one call, handed back when it goes
struct ImageLease {
  BufPool &pool;
  void *p = nullptr;
  size_t bytes = 0;
  ImageLease(BufPool &pl, size_t n) : pool(pl) {
    p = pool.take_image(n, &bytes);
    if (!p) throw SlgError(SLG_ERR_OOM, "pinned staging image: hipHostMalloc failed");
  }
  ~ImageLease() { pool.give_image(p, bytes); }
  ImageLease(const ImageLease &) = delete;
  ImageLease &operator=(const ImageLease &) = delete;
};

// hipMalloc that drains `pool` (may be null) and tries once more when the device is out of memory
inline void *device_alloc(size_t n, BufPool *pool) {
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

// the calling thread on device `dev` for a scope, without error checks (destructors, destroy calls)
struct DeviceScope {
  int prev = -1;
  explicit DeviceScope(int dev) {
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(dev);
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

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
  DevBuf(DevBuf &&o) noexcept { swap(o); }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      release();
      swap(o);
    }
    return *this;
  }
  void swap(DevBuf &o) noexcept {
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
    std::swap(pool, o.pool);
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
  uint32_t dim = 0, n_rows = 0;
};
struct VecFieldHost {
  uint32_t dim = 0;
  int32_t metric = 0;
  std::vector<std::shared_ptr<VecSegStore>> per_seg;
  DevBuf d_vsegs;  // slg::VecSegDev[n_segs] of the state this object belongs to
};

// the bf16 copy of a vector field (slg_index_quantize_vector_field; field 0 too): per segment the shared copy of
// its store (null: the segment has no vectors in the field), in the store's row order
struct VecCopySeg {
  DevBuf rows, norms;  // u16[n_rows * dim_pad] bf16, zero-padded rows | f32[n_rows] squared norms of the f32 rows
  uint32_t n_rows = 0, dim = 0, dim_pad = 0;
};
struct VecCopyField {
  std::vector<std::shared_ptr<VecCopySeg>> per_seg;
  DevBuf d_csegs;  // slg::VecCopyDev[n_segs] of the state this object belongs to
};

// the inverted-file lists of a vector field (slg_index_cluster_vector_field; field 0 too): per segment the shared
// lists of its store (null: the segment is unclustered, or has no vectors in the field)
struct VecListSeg {
  DevBuf list_begin, docs, centroids, iota;  // u32[n_lists + 1] | u32[n_listed] | f32[n_lists * dim] | u32[n_lists] 0, 1, ..
  uint32_t n_lists = 0, dim = 0, n_listed = 0, max_len = 0;
};
struct VecListField {
  std::vector<std::shared_ptr<VecListSeg>> per_seg;
  // the tables of the state this object belongs to: the lists, the centroid tables as pseudo-segments of the exact
  // scan (a "doc" = a list) with their tombstone-free segment descriptors and flat list bases, the unclustered segments
  DevBuf d_lsegs, d_csegs, d_psegs, d_list_base, d_uncl;
  uint32_t total_lists = 0, max_len = 0, n_uncl = 0, uncl_slots = 0;
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

// a registered aggregation column (slg_index_add_agg_field_*): per segment the CSR on the device; null = the
// field predates the segment (slg_index_add_segment).  Registration scans the values once: the finite
// minimum and maximum (a histogram's dense id range follows from them) and whether a non-finite one exists
struct AggColumn {
  DevBuf offs, vals;   // offs empty: every doc of the segment has exactly one value (vals[doc])
  size_t n_vals = 0;   // values in vals
  // what registration saw in this segment's values (numeric columns); the field's own facts are these folded over
  // the segments it holds (AggFieldData::refold), so that they follow slg_index_remove_segment
  bool any_value = false, non_finite = false, i64_rounded = false;
  double vmin = 0.0, vmax = 0.0;
};
// the value ranks of a numeric field (slg_index_rank_agg_field): the dictionary of its distinct values, shared by
// the states that hold the field
struct AggRankDict {
  std::vector<uint64_t> keys;  // sorted order-preserving keys of the distinct values (agg_f64_key)
  DevBuf vals;                 // f64[keys.size()]: the values, in the same order
};
struct AggFieldData {
  int kind = 0;  // 1 numeric (f64 values), 2 keyword (u32 ordinals)
  uint32_t n_ords = 0;
  bool any_value = false, non_finite = false;
  double vmin = 0.0, vmax = 0.0;  // over the finite values, when any_value
  // the numeric column came from slg_index_add_agg_field_i64 (a RANGE_I64 filter leaf asks for it); some value of
  // it lay beyond +-2^53 and was rounded by `as f64`
  bool from_i64 = false, i64_rounded = false;
  std::vector<std::shared_ptr<AggColumn>> per_seg;
  // set by slg_index_rank_agg_field (numeric fields): the dictionary, and per segment u32[n_vals] beside vals
  std::shared_ptr<AggRankDict> dict;
  std::vector<std::shared_ptr<DevBuf>> ranks;  // [per_seg.size()]; null = no ranks for that segment
  // any_value / vmin / vmax / non_finite / i64_rounded from the columns of the segments held now: what a
  // registration over exactly these segments would have recorded
  void refold() {
    any_value = non_finite = i64_rounded = false;
    vmin = vmax = 0.0;
    for (const auto &c : per_seg) {
      if (!c) continue;
      non_finite = non_finite || c->non_finite;
      i64_rounded = i64_rounded || c->i64_rounded;
      if (!c->any_value) continue;
      vmin = any_value ? std::min(vmin, c->vmin) : c->vmin;
      vmax = any_value ? std::max(vmax, c->vmax) : c->vmax;
      any_value = true;
    }
  }
};

// a registered nested path (slg_index_add_nested_path): per segment the docs' first objects, the object -> doc
// table and the parent lists on the device; null = the path predates the segment (slg_index_add_segment)
struct NestedPathSeg {
  DevBuf base, obj_doc;      // u32[n_docs + 1] | u32[n_objects]
  DevBuf par_offs, parents;  // u32[n_docs + 1] | u32[]; both empty: nothing binds
  uint32_t n_objects = 0;
  size_t device_bytes() const { return base.bytes + obj_doc.bytes + par_offs.bytes + parents.bytes; }
};
struct NestedPathData {
  int parent = -1;  // the path id one level up, or -1
  std::vector<std::shared_ptr<NestedPathSeg>> per_seg;
};
// a registered nested value column (slg_index_add_nested_field_*): per segment its two offset arrays and the
// values; null = the field predates the segment
struct NestedColSeg {
  DevBuf doc_offs, obj_offs, vals;  // doc_offs empty: the segment has no value (registered with NULL)
  size_t device_bytes() const { return doc_offs.bytes + obj_offs.bytes + vals.bytes; }
};
struct NestedFieldData {
  int path = 0;
  int kind = 0;  // 1 f64, 2 i64, 3 keyword ordinals
  uint32_t n_ords = 0;
  std::vector<std::shared_ptr<NestedColSeg>> per_seg;
};

// the positions of a segment's postings (slg_index_set_positions): shared by the states that hold them
struct PosStore {
  DevBuf offs;  // u32[P + 1] in the unpadded posting order
  DevBuf pos;   // u32[offs[P]]
};

// the term dictionary of a segment (slg_index_set_terms): the host copy the merge of slg_expand_batch reads and
// what the scan reads on the device; shared by the states that hold it
struct TermStore {
  slgexpand::Dict dict;
  DevBuf bytes, offs, map, nchars;  // sorted key bytes | u32[n + 1] | u32[n] sorted position -> term id | u8[n]
  // slg_suggest_batch: the posting-list length of the key at each sorted position (the segment's term_offsets as
  // staged, whatever is deleted), and how many of the keys in front of each position have one above 0
  std::vector<uint32_t> df;         // [n]
  std::vector<uint32_t> nonzero;    // [n + 1]
  DevBuf d_df;                      // u32[n]
  size_t device_bytes() const { return bytes.bytes + offs.bytes + map.bytes + nchars.bytes + d_df.bytes; }
};

// a registered text field (slg_index_add_text_field): per segment the docs' texts on the device, shared by the
// states that hold them; null = the segment has no text in the field (it passed NULL, or was added later)
struct TextSegStore {
  DevBuf bytes, offs, non_ascii;  // the texts padded by 16 bytes | u64[n_docs + 1] | one bit per doc
  uint32_t n_docs = 0;
  size_t device_bytes() const { return bytes.bytes + offs.bytes + non_ascii.bytes; }
};
struct TextFieldHost {
  std::vector<std::shared_ptr<TextSegStore>> per_seg;
  DevBuf d_tsegs;  // slg::TextSegDev[n_segs] of the state this object belongs to
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
  std::map<uint32_t, std::shared_ptr<VecCopyField>> vcopies;  // by field id (0 too); own objects, shared copies
  std::map<uint32_t, std::shared_ptr<VecListField>> vlists;   // the same for the inverted-file lists
  std::vector<std::shared_ptr<FilterData>> filters;    // slot = filter id; null = free
  std::vector<const uint32_t *> reject_host;           // flattened [filter * n_segs + seg] device pointers
  DevBuf d_reject_table;                               // the same table on the device
  std::map<int, std::shared_ptr<SortFieldData>> sort_fields;  // by id (ids are not reused)
  std::map<int, std::shared_ptr<AggFieldData>> agg_fields;    // by id (ids are not reused)
  std::map<int, std::shared_ptr<NestedPathData>> nested_paths;    // by id (ids are not reused)
  std::map<int, std::shared_ptr<NestedFieldData>> nested_fields;  // by id (ids are not reused)
  std::vector<std::shared_ptr<PosStore>> positions;          // [n_segs]; null = the segment has none
  DevBuf d_pos_segs;                                          // slg::PosSegDev[n_segs]
  std::vector<std::shared_ptr<TermStore>> terms;              // [n_segs]; null = the segment has no dictionary
  DevBuf d_term_segs;                                         // slg::ExpandSegDev[n_segs]
  DevBuf d_suggest_segs;                                      // slg::SuggestSegDev[n_segs]
  std::map<int, std::shared_ptr<TextFieldHost>> text_fields;  // by id (ids are not reused); own objects, shared stores
  ~IndexState() {
    // kernels of already-destroyed batches, or rerank calls on the index stream, may still read the
    // tables: retiring a state is rare (one per update), so wait for the device once
    DeviceScope on(device);
    (void)hipDeviceSynchronize();
  }
  // a filter id a query may name: registered, with a bitmap for every segment of this state
  bool filter_usable(size_t f) const {
    return f < filters.size() && filters[f] && filters[f]->complete() && filters[f]->per_seg.size() == segs.size();
  }
};

}  // namespace slghost

struct slg_index {
  // work buffers of finished batches.  Shared with the batches (a batch that outlives the index
  // still returns its buffers somewhere valid); declared first: destroyed last
  slghost::BufPool pool;
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
  std::shared_ptr<const slghost::IndexState> state;  // the current state (under mu)
  std::atomic<uint64_t> generation{0};               // = state->generation, readable without the lock
  std::mutex mu;
  std::mutex update_mu;  // serialises slg_index_update_* / add_filter / add_vector_field (taken before mu)
  int next_sort_field = 0;  // (under update_mu) sort field ids are never handed out again
  int next_agg_field = 0;   // (under update_mu) the same for aggregation fields
  int next_text_field = 0;  // (under update_mu) and for text fields
  int next_nested_path = 0, next_nested_field = 0;  // (under update_mu) and for nested paths and nested fields
  // profiling of the scoring kernel
  bool profile = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
  size_t prof_used = 0;
  // set by a scoring wave that had to give up on a round (chunk-loop guard): checked at fetch
  slghost::DevBuf d_error_flag;
  // work space of slg_vector_search_batch* (under mu; used on `stream` only, so a call that grows it
  // frees the old block with hipFree, which waits for the device)
  slghost::DevBuf vs_scratch;
  std::shared_ptr<const slghost::IndexState> snapshot() {
    std::lock_guard<std::mutex> lk(mu);
    return state;
  }
};

// Every device buffer of a batch, and nothing else: slg_index_destroy detaches a batch that outlives the index by
// move-assigning a fresh one of these over it (slghost::release_batch_buffers), so a DevBuf declared here is
// released there without being named anywhere.  The kinds they belong to are described at slg_batch's scalars.
struct slg_batch_buffers {
  using DevBuf = slghost::DevBuf;
  DevBuf d_desc;                     // packed descriptors
  DevBuf d_bounds, d_rdoc, d_slice_tk, d_slice_doc, d_q_scored, d_slice_desc;
  DevBuf d_q_filter;       // [nq] 0 = none, f + 1 (select_topk_kernel); empty when unfiltered
  DevBuf d_cand, d_slice_cbeg, d_slice_ccnt;  // cand_mode: candidates + select_topk_kernel
  DevBuf d_sort_cols;  // slg::SortColDev[kSortMaxParts * n_segs]
  DevBuf d_matched;    // u64[nq] accepted docs (the batches PrepareRequest::counts_matched names, and scan batches)
  DevBuf d_cursor;  // u32[nq * slg::kCursorStride]: has_cursor, then the key words of the select kernel
  DevBuf d_seen;    // u32[nq] the cursor's key was seen
  DevBuf d_out;  // the result block (slghost::ResultBlock) + the error word
  DevBuf d_stamps;  // SLG_STAMPS diagnostic builds
  DevBuf d_blk_skip;  // block skipping: postings of non-essential lists that were never loaded (u64)
  // index-sharded runs (slg_batch_run_sharded): the gathered result blocks of all ranks and the merged
  // top-k, a result block too
  DevBuf d_gather, d_merged;
  DevBuf d_q_cand;               // slg_batch::q_cand on the device
  DevBuf d_hy_keys, d_hy_work;   // the gathered keys of a range of queries; clause lists, counts, sort space
  DevBuf d_agg_desc;                 // slg::AggNodeDev[n_nodes], slg::ColumnDev[n_nodes * n_segs], then the rank columns
  DevBuf d_agg_counts, d_agg_stats;  // u32[nq * count_cells], slg::AggStatDev[nq * stats_cells]
  DevBuf d_agg_values, d_agg_scratch;         // u64[nq * value_cells], u32[nq * scratch_words]
  DevBuf d_rs_desc;  // slg::RescoreQuery[nq], then slg::RescoreTerm[total x n_segs]
  DevBuf d_rs_side;  // first-pass score | rescore score | rescored flag, [nq * k] each
  DevBuf d_bool_desc;        // slg::BoolQuery[nq], then slg::BoolTerm rows per (query, segment)
  DevBuf d_phrase_desc;      // slg::PhraseQuery[nq], slg::PhraseVar[phrase_vars], slg::PhraseTerm[phrase_terms]
  DevBuf d_booltree_desc;    // slg::BoolTreeQuery[nq], BoolTreeNode[bt_nodes], BoolTerm[bt_terms], bitmap addresses
                             // [bt_filters], then the filter rows
  DevBuf d_fscore_desc;      // slg::FscoreQuery[nq], FscoreFn[fscore_fns], ColumnDev[fscore_cols], bitmap addresses
  DevBuf d_script_desc;           // slg::ScriptQuery[nq], ScriptInstr[script_instrs], ColumnDev[fields][n_segs]
  DevBuf d_cl_desc;  // slg::ColumnDev[n_segs], then slg::SortColDev[kSortMaxParts * n_segs] of the inner sort
  DevBuf d_cl_side;  // the arrays of slg_batch_fetch_collapse, back to back in its argument order
  DevBuf d_th_desc;     // slg::TopHitsNodeDev[n_nodes], then slg::SortColDev[n_nodes][kSortMaxParts * n_segs]
  DevBuf d_th_out;      // doc | seg | score [nq * hit_cells], count [nq * list_cells], status [nq], the error word
  DevBuf d_th_entries, d_th_cursors;  // uint2[nq * max_entries], u32[nq * cursor_words]
  DevBuf d_cp_desc;    // slg::AggNodeDev[n_children], ColumnDev[n_children * n_segs], ColumnDev[n_sources * n_segs],
                       // slg::CompositeSourceDev[n_sources]
  DevBuf d_cp_ranks;   // u32: the ord_rank of every terms source that has one, back to back
  DevBuf d_cp_lower;   // u64[nq] the inclusive lower bounds (slg_batch_set_composite_after)
  DevBuf d_cp_out;     // u64 keys [nq * size], then u32 n_buckets [nq], has_more [nq], the error word
  DevBuf d_cp_counts, d_cp_stats;  // u32[nq * cp_count_cells], slg::AggStatDev[nq * cp_stats_cells]
  DevBuf d_tb_desc;   // slg::TermBucketNodeDev[n], ColumnDev[n * n_segs], per node AggNodeDev[], ColumnDev[] of its children
  DevBuf d_tb_ranks;  // u32: ord_rank and its inverse of every ranked node, back to back
  DevBuf d_tb_bg;     // u32 [n_segs][n_ords + 1] per distinct (field, background filter): bg_count_kernel's tables
  DevBuf d_tb_fg, d_tb_bgsum, d_tb_bits;  // u32 / u64 [nq * tb_fg_cells], u32 [nq * tb_bits_words]
  DevBuf d_tb_out;    // the arrays of slg_batch_fetch_term_buckets and the error word (slg_termbuckets.hip: OutBlock)
  DevBuf d_tb_sorted; // u32 [nq * rows] the kept ordinals in ordinal order, then [nq * rows] the row of each
  DevBuf d_tb_counts, d_tb_stats;  // u32[nq * tb_count_cells], slg::AggStatDev[nq * tb_stats_cells]
};

struct slg_batch : slg_batch_buffers {
  slg_index *idx = nullptr;
  std::shared_ptr<const slghost::IndexState> snap;  // the index state the batch was prepared on
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
  bool last_sharded = false;         // the last run was slg_batch_run_sharded*: the rows a caller holds are the merged ones
  // slg_batch_explain (slg_explain.hip): the sub-query of every (query, segment) pair, [nq * n_segs], 0xFFFFFFFF where
  // the pair has none; the most term rows (all segments) of one query.  From the plan, at prepare
  std::vector<uint32_t> ex_q_seg_sq;
  uint32_t ex_max_table = 0;
  bool own_stream_set = false;       // slg_batch_set_stream: run on `stream` instead of the index's
  hipStream_t stream = nullptr;
  const slg::RoundQuery *d_sq = nullptr;
  const slg::TermRef *d_terms = nullptr;
  const uint32_t *d_slice_sq = nullptr;
  const uint32_t *d_slice_seg = nullptr;
  const uint32_t *d_slice_order = nullptr;
  const slg::QueryRef *d_queries = nullptr;
  const uint32_t *d_bnd_coarse = nullptr;
  bool cand_mode = false;  // uniform kernel, k > 256: candidates + select_topk_kernel
  // field-sorted batch (slg_batch_prepare_sorted): candidates of every matched doc + select_sorted_kernel
  bool sorted = false;
  uint32_t score_k = 0;  // k the scoring kernel runs with (a sorted batch: slgplan::planning_k)
  uint32_t n_sort_parts = 0, sort_score_parts = 0, sort_desc_parts = 0;
  // cursor batch (slg_batch_prepare_after): score order (!sorted: select_topk_kernel<true>) or a field sort
  // (select_sorted_kernel<true>)
  bool after = false;
  uint32_t *d_out_doc = nullptr, *d_out_seg = nullptr, *d_out_count = nullptr;
  float *d_out_score = nullptr;
  // index-sharded runs (slg_batch_run_sharded): d_gather and d_merged
  slg_shard_group *shard_group = nullptr;  // the group of the last sharded run (timing goes there)
  hipEvent_t ev_shard[4] = {nullptr, nullptr, nullptr, nullptr};  // start | local kernels done | gathered | merged
  bool shard_timed = false;
  uint64_t n_postings_nonessential = 0;  // postings of the pruning-classified (non-essential) lists
  // hybrid text + vector batch (slg_batch_prepare_hybrid): planned as a sorted batch (candidates of every
  // matched doc), run as a score page without a cursor; slg_batch_hybrid_device then reads the candidates
  bool hybrid = false;
  std::vector<uint64_t> q_cand;  // [nq + 1] first candidate slot of each query (d_q_cand: the same on the device)
  // aggregation batch (slg_batch_prepare_aggs): planned as a sorted batch, run in score order or under its
  // sort spec; agg_kernel then fills the tables from the candidates (slg_aggs.hip)
  bool aggs = false;
  slg_agg_spec agg_spec{};
  std::vector<slg_agg_layout> agg_layout;  // [n_nodes]
  uint32_t agg_count_cells = 0, agg_stats_cells = 0;
  bool agg_lds = false;              // the tables fit SLG_AGG_LDS_BYTES
  // value nodes (cardinality, percentiles, percentile_ranks): agg_values_kernel behind agg_kernel
  uint32_t agg_value_nodes = 0, agg_value_cells = 0, agg_card_words = 0, agg_scratch_words = 0, agg_pct_lds = 0;
  bool agg_walk1 = false, agg_x_lds = false;  // a cardinality / percentile_ranks node; cells and bitmaps fit LDS
  bool agg_ext = false;                       // a date_histogram or filter node: the kernels that hold those paths
  // rescore batch (slg_batch_prepare_rescore): rescore_kernel runs behind the first pass's last kernel and
  // rewrites the first rows of every query in place (slg_rescore.hip)
  bool rescore = false;
  uint32_t rs_lds_rows = 0, rs_max_table = 0;  // LDS rows (>= every window, even) and table entries of the launch
  // bool batch (slg_batch_prepare_bool): planned as a sorted batch, run in score order or under its sort spec;
  // bool_filter_kernel runs between the scoring kernel and the select and drops the candidates the clause
  // tables reject (slg_bool.hip)
  bool boolean = false;
  uint32_t bool_groups = 0;  // groups of all queries (0: no query has a clause table, nothing is launched)
  // phrase batch (slg_batch_prepare_phrase): a bool batch (boolean is set, d_bool_desc holds the term groups'
  // tables) whose clause tables also have phrase groups; phrase_filter_kernel runs in bool_filter_kernel's
  // place (slg_phrase.hip)
  bool phrase = false;
  uint32_t phrase_vars = 0, phrase_terms = 0;  // entries of the two tables behind the PhraseQuery records
  // tree batch (slg_batch_prepare_bool_tree): planned and run as a bool batch; booltree_filter_kernel runs in
  // bool_filter_kernel's place and drops the candidates the query's matcher tree rejects (slg_booltree.hip)
  bool booltree = false;
  uint32_t bt_nodes = 0, bt_terms = 0, bt_filters = 0;  // entries of the tables (bt_nodes 0: nothing is launched)
  // function_score batch (slg_batch_prepare_fscore): planned as a sorted batch, run in score order or under its
  // sort spec; fscore_kernel runs between the scoring kernel and the select, rewrites every candidate's score and
  // drops the candidates below min_score (slg_fscore.hip)
  bool fscore = false;
  uint32_t fscore_work = 0;  // queries with work (0: nothing is launched)
  bool fscore_full = false;  // some function needs ln / log1p / log2 / pow: the full instantiation
  uint32_t fscore_fns = 0, fscore_cols = 0;  // entries of the two tables behind the FscoreQuery records
  // script_score batch (slg_batch_prepare_script): planned as a function_score batch is; script_kernel runs between
  // the scoring kernel and the select — alone, in front of the fscore stage (script_first) or behind it — rewrites
  // every candidate's score and drops the candidates whose script gives none (slg_script.hip)
  bool script = false, script_first = false;
  uint32_t script_work = 0;       // queries with a program (0: nothing is launched)
  uint32_t script_max_depth = 0;  // the deepest stack of the batch's programs
  uint32_t script_instrs = 0;     // entries of the instruction table behind the ScriptQuery records
  // scan batch (slg_batch_prepare_scan): no scored term, so no sub-queries, terms or rounds; scan_kernel fills the
  // candidate regions in the place of the partition and scoring kernels and counts d_q_scored and d_matched
  // (slg_scan.hip).  d_desc holds slg::ScanSlice[n_slices], ScanQuery[nq], ColumnDev[fields][n_segs], then the
  // query and slice-segment tables every batch has
  bool scan = false;
  bool scan_full = false;  // some query needs ln / log1p: the full instantiation
  // collapse batch (slg_batch_prepare_collapse): a plain, sorted or cursor batch; collapse_kernel runs behind its
  // last kernel and fills the side arrays from each query's rows, which it leaves as they are (slg_collapse.hip)
  bool collapse = false;
  uint32_t cl_groups = 0, cl_from = 0, cl_size = 0;  // group_limit, inner_from, inner_size
  uint32_t cl_lds_rows = 0;                          // rows the kernel's LDS arrays hold: a power of two >= k
  uint32_t cl_parts = 0, cl_score_parts = 0, cl_desc_parts = 0;  // the inner sort (0 parts: the batch's own order)
  // top_hits batch (slg_batch_prepare_top_hits): an aggregation batch, or a plain / sorted one planned as such;
  // top_hits_kernel runs behind agg_kernel and fills the lists from the candidates (slg_tophits.hip)
  bool top_hits = false;
  slg_top_hits_spec th_spec{};
  std::vector<slg_top_hits_layout> th_layout;  // [n_nodes]
  uint32_t th_hit_cells = 0, th_list_cells = 0;  // of one query
  uint32_t th_max_entries = 0;                   // run slots of one query
  uint32_t th_cursor_words = 0, th_lds_cursors = 0;  // cursors of one query in device memory / in LDS
  bool th_ext = false;  // a date_histogram or filter parent: the instantiation that holds those paths
  // composite batch (slg_batch_prepare_composite): an aggregation batch, or a plain / sorted one planned as such;
  // composite_select_kernel and composite_collect_kernel run behind agg_kernel (slg_composite.hip).  The composite's
  // tables are its own: agg_kernel's keep their stride, slg_batch_fetch_aggs puts the two side by side
  bool composite = false;
  slg_composite_spec cp_spec{};  // (ord_rank: not kept, the ranks are on the device)
  slg_composite_layout cp_layout{};
  uint32_t cp_count_cells = 0, cp_stats_cells = 0;  // of one query: `size` count cells, then the children's tables
  uint32_t cp_cap = 0;        // entries of one wave's key set in composite_select_kernel
  bool cp_lds = false, cp_ext = false;  // the tables fit SLG_AGG_LDS_BYTES; a date_histogram or filter child
  size_t cp_cols_off = 0, cp_src_cols_off = 0, cp_src_off = 0;  // byte offsets into d_cp_desc
  // term bucket batch (slg_batch_prepare_term_buckets): an aggregation batch, or a plain / sorted one planned as
  // such; term_bucket_count_kernel, _select_kernel and (a node with children) _collect_kernel run behind agg_kernel
  // (slg_termbuckets.hip).  The children's cells lie behind the aggregation spec's in the arrays of
  // slg_batch_fetch_aggs, in tables of their own on the device
  bool term_buckets = false;
  slg_term_bucket_spec tb_spec{};  // (ord_rank: not kept, the ranks are on the device)
  slg_term_bucket_layout tb_layout{};
  uint32_t tb_fg_cells = 0, tb_bits_words = 0;      // of one query: cells of fg / bgsum, presence words
  uint32_t tb_count_cells = 0, tb_stats_cells = 0;  // of one query: the children's tables of every node
  bool tb_lds = false;  // the count walk's fg cells (4 B each) fit SLG_AGG_LDS_BYTES
  struct TbNodeTables {  // a node with children: its tables in a query's term bucket rows, its part of d_tb_desc
    uint32_t cnt_off = 0, st_off = 0, count_cells = 0, stats_cells = 0;
    size_t nodes_off = 0, cols_off = 0;
    bool lds = false, ext = false;
  };
  TbNodeTables tb_tables[SLG_MAX_TERM_BUCKET_NODES];
  size_t tb_cols_off = 0;  // byte offset of the nodes' columns in d_tb_desc
};

namespace slghost __attribute__((visibility("hidden"))) {

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

inline int kregs_for(uint32_t k) {
  if (k <= 64) return 1;
  if (k <= 128) return 2;
  if (k <= 256) return 4;
  if (k <= 512) return 8;
  return 16;
}

// Waiting for a stream is the blocking hipStreamSynchronize.  (Polling hipStreamQuery first — to spare a
// small batch the sleep / wake-up of the blocking wait — was built and measured: with 8 caller threads
// polling, config 2's host-inclusive rate fell from 11M to 2.2M queries/s and fetch + destroy grew from
// 0.28 to 1.36 ms per batch: the query takes a runtime lock the other threads' launches and copies need.)
inline hipError_t wait_stream(hipStream_t st) { return hipStreamSynchronize(st); }

// the stream a batch runs on (the caller holds ix->mu) ...
inline hipStream_t batch_stream(const slg_batch *b) { return b->own_stream_set ? b->stream : b->idx->stream; }
// ... and the same for a caller that goes on to wait for it: read under the index mutex, which is NOT held
// while waiting, so other host threads keep launching their batches
inline hipStream_t locked_stream(const slg_batch *b) {
  std::lock_guard<std::mutex> lk(b->idx->mu);
  return batch_stream(b);
}

// The result block of a batch of nq queries at k: doc[nq*k] | seg[nq*k] | score[nq*k] | count[nq], 32-bit
// words in one allocation, so that one copy (to the host, or an all-gather between ranks) moves a batch's
// results.  A batch's own block (slg_batch::d_out) carries one more word behind it: the index's error word
// as the batch's last kernel saw it (MergeParams::out_flag).
struct ResultBlock {
  size_t n, nq;  // n = nq * k entries per array
  ResultBlock(uint32_t nq_, uint32_t k) : n((size_t)nq_ * k), nq(nq_) {}
  size_t words() const { return 3 * n + nq; }
  size_t words_with_flag() const { return words() + 1; }
  uint32_t *doc(uint32_t *base) const { return base; }
  uint32_t *seg(uint32_t *base) const { return base + n; }
  float *score(uint32_t *base) const { return reinterpret_cast<float *>(base + 2 * n); }
  uint32_t *count(uint32_t *base) const { return base + 3 * n; }
  uint32_t *flag(uint32_t *base) const { return base + words(); }
  // a host copy of the block to the caller's arrays
  void unpack(uint32_t *host_block, uint32_t *out_doc, uint32_t *out_seg, float *out_score,
              uint32_t *out_count) const {
    if (n) {
      std::memcpy(out_doc, doc(host_block), n * 4);
      std::memcpy(out_seg, seg(host_block), n * 4);
      std::memcpy(out_score, score(host_block), n * 4);
    }
    std::memcpy(out_count, count(host_block), nq * 4);
  }
};

// The host arrays of one call staged through pooled device buffers on one stream (the host-array forms
// of rerank and vector search): up() allocates a buffer of n elements and, src given, queues its upload;
// down() queues the copy back if the caller wants the array.  The destructor waits for the stream on
// every exit before the buffers go back to the pool, so no block is reused while a queued copy or kernel
// may still touch it.
struct Staging {
  BufPool *pool;
  hipStream_t st;
  std::vector<DevBuf> bufs;
  Staging(BufPool *pl, hipStream_t s) : pool(pl), st(s) { bufs.reserve(16); }
  ~Staging() { (void)hipStreamSynchronize(st); }
  template <typename T>
  T *up(const T *src, size_t n) {
    bufs.emplace_back();
    bufs.back().alloc_pooled(pool, n * sizeof(T));
    if (src && n) SLG_HIP(hipMemcpyAsync(bufs.back().p, src, n * sizeof(T), hipMemcpyHostToDevice, st));
    return bufs.back().as<T>();
  }
  template <typename T>
  void down(T *dst, const T *src, size_t n) {
    if (dst && n) SLG_HIP(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, st));
  }
};

// ---- defined in one unit, used by others -------------------------------------------------------
// slg_batch.hip: give back everything a batch holds on the device, its shard events included (slg_index_destroy,
// on the index's device, its pool still alive: the blocks go there or, past its cap, to the runtime).  The
// batch's scalar facts stay: slg_batch_info and the *_layout calls still answer
void release_batch_buffers(slg_batch *b);
// slg_batch.hip: the merge of several ranks' (or shards') rows
void launch_shard_merge(const slg::ShardMergeParams &mp, hipStream_t st);
// slg_batch.hip: a sort spec against an index state: the column table [kSortMaxParts * n_segs] (part p of segment
// s at p * n_segs + s; null rows for `_score` parts and beyond the spec) and the bits of the `_score` and the
// descending parts.  Throws SLG_ERR_INVALID "<prefix>unknown sort field id in <part>I" and "<prefix>sort field N
// has no column for segment S (added after the field was registered)"
struct SortBinding {
  std::vector<slg::SortColDev> cols;
  uint32_t score_parts = 0, desc_parts = 0;
};
SortBinding bind_sort(const IndexState &S, const slg_sort_spec &spec, const std::string &prefix, const std::string &part);

// slg_batch.hip: every slg_batch_prepare* is one PrepareRequest.  The query arrays, and one member per batch
// kind; a kind that was asked for and its spec travel together, so a kind asked for with a NULL spec still
// reaches its check.  (hybrid and aggs plan as slg_batch_prepare_plans / _sorted with BatchIn::sorted)
template <typename T>
struct Asked {
  bool on = false;
  const T *spec = nullptr;
};
struct PrepareRequest {
  slg_index *ix;
  uint32_t nq;
  const uint32_t *q_offsets, *q_term_ids;
  const float *q_weights;
  const slg_score_plans *plans;
  const int32_t *q_filter;
  uint32_t k;
  int strategy;
  Asked<slg_sort_spec> sort;      // off: score order
  Asked<slg_sort_cursor> cursor;  // slg_batch_prepare_after
  bool hybrid = false;            // slg_batch_prepare_hybrid
  Asked<slg_agg_spec> aggs;
  Asked<slg_rescore_spec> rescore;
  Asked<slg_bool_spec> boolean;   // a phrase batch: on, its spec may be NULL (no term groups)
  Asked<slg_phrase_spec> phrase;
  Asked<slg_bool_tree_spec> booltree;
  Asked<slg_fscore_spec> fscore;
  Asked<slg_script_spec> script;  // slg_batch_prepare_script (with fscore: the two stages, in script_order)
  int script_order = 0;           // SLG_SCRIPT_OUTER / _INNER
  Asked<slg_collapse_spec> collapse;
  Asked<slg_top_hits_spec> top_hits;  // slg_batch_prepare_top_hits (aggs: on when its spec is given)
  Asked<slg_composite_spec> composite;  // slg_batch_prepare_composite (aggs: on when its spec is given)
  Asked<slg_term_bucket_spec> term_buckets;  // slg_batch_prepare_term_buckets (aggs: on when its spec is given)
  // the batch counts the docs its select, agg_kernel or a kernel behind them accepts (slg_batch::d_matched) ...
  bool counts_matched() const {
    return sort.spec != nullptr || cursor.on || aggs.on || top_hits.on || composite.on || term_buckets.on;
  }
  // ... and is planned with candidates of every matched doc (BatchIn::sorted): those, and the kinds whose kernels
  // between scoring and select read or rewrite every candidate
  bool plans_every_match() const {
    return counts_matched() || hybrid || boolean.on || booltree.on || fscore.on || script.on;
  }
};
// a spec that is a kind of its own only when it is given (the sort of a bool, phrase, cursor or agg batch)
template <typename T>
Asked<T> if_given(const T *spec) {
  return Asked<T>{spec != nullptr, spec};
}
slg_batch *prepare_impl(const PrepareRequest &r);

// ---- what slg_batch_prepare_scan (slg_scan.hip) shares with prepare_impl -----------------------------------------
// the argument checks of a sort spec (null: score order), made before planning
inline void check_sort_spec(const slg_sort_spec *sort) {
  if (!sort) return;
  if (sort->n_parts > SLG_MAX_SORT_PARTS) throw SlgError(SLG_ERR_UNSUPPORTED, "more than SLG_MAX_SORT_PARTS sort parts");
  SLG_REQUIRE(sort->n_parts >= 1, "a sort spec needs at least one part");
  for (uint32_t i = 0; i < sort->n_parts; i++)
    SLG_REQUIRE(sort->order[i] == SLG_ORDER_ASC || sort->order[i] == SLG_ORDER_DESC, "unknown sort order");
}
// which filter ids of a state a query may name, as the planners read it
inline std::vector<char> filter_liveness(const IndexState &S) {
  std::vector<char> live(S.filters.size());
  for (size_t f = 0; f < live.size(); f++) live[f] = S.filter_usable(f);
  return live;
}
// slg_batch.hip: what the select kernels read and write, onto the device: the planned filter words (empty: no
// query is filtered), the columns of the sort (null: score order), the matched counts if the batch has them, and
// the result block
void attach_select_buffers(slg_batch *b, const std::vector<uint32_t> &q_filter, const slg_sort_spec *sort,
                           const SortBinding &sorting, bool counts_matched);
// the frame of a prepare call: build(b) checks, plans, allocates b and fills it, throwing at the first fault; the
// finished batch is registered with its index, a half-built one destroyed (the thread's error kept)
template <typename F>
slg_batch *prepare_guarded(F &&build) {
  slg_batch *b = nullptr;
  const int rc = guarded([&] {
    build(b);
    std::lock_guard<std::mutex> lk(b->idx->mu);
    b->idx->live.push_back(b);
  });
  if (rc != SLG_OK) {
    KeepLastError keep;
    delete b;
    return nullptr;
  }
  return b;
}
// the host arrays of a one-call search: the rows, and what the batch's kind adds to them (null: not asked for)
struct HostOut {
  uint32_t *doc, *seg;
  float *score;
  uint32_t *count;
  slg_stats *stats = nullptr;
  uint64_t *matched = nullptr;
  uint8_t *seen = nullptr;
  uint64_t *agg_counts = nullptr;  // (an aggregation batch)
  slg_agg_stats *agg_stats = nullptr;
  uint64_t *agg_values = nullptr;
  float *first_score = nullptr, *rescore_score = nullptr;  // (a rescore batch)
  uint32_t *rescored = nullptr;
  void *const *collapse = nullptr;  // (a collapse batch) the 14 arrays of slg_batch_fetch_collapse, in its order
  uint32_t *th_doc = nullptr, *th_seg = nullptr, *th_count = nullptr, *th_status = nullptr;  // (a top_hits batch)
  float *th_score = nullptr;
  uint64_t *cp_keys = nullptr;  // (a composite batch)
  uint32_t *cp_n_buckets = nullptr, *cp_has_more = nullptr;
  uint32_t *tb_ords = nullptr, *tb_n_buckets = nullptr;  // (a term bucket batch)
  uint64_t *tb_doc_counts = nullptr, *tb_bg_counts = nullptr, *tb_score_bits = nullptr, *tb_node_dc = nullptr,
           *tb_node_bg = nullptr;
};
// slg_batch.hip: a prepared batch (null: prepare failed and set the thread's error) run to the caller's host arrays
// and destroyed: the first error is the one reported
int run_to_host(slg_batch *b, const HostOut &o);

// the tables of a batch kind: host arrays back to back as one image in a pooled device buffer, one copy
struct ImagePart {
  const void *p;
  size_t bytes;
};
template <typename T>
ImagePart image_part(const std::vector<T> &v) {
  return ImagePart{v.data(), v.size() * sizeof(T)};
}
inline void upload_image(DevBuf &dst, BufPool *pool, std::initializer_list<ImagePart> parts) {
  std::vector<unsigned char> image;
  for (const ImagePart &pt : parts)
    image.insert(image.end(), static_cast<const unsigned char *>(pt.p), static_cast<const unsigned char *>(pt.p) + pt.bytes);
  dst.alloc_pooled(pool, image.size());
  if (!image.empty()) SLG_HIP(hipMemcpy(dst.p, image.data(), image.size(), hipMemcpyHostToDevice));
}

// One host block of `words` 32-bit words for ONE D2H copy of a batch's results: a small block is pageable memory,
// a large one a pinned image of the index's pool (why, with the measurement: slg_batch_fetch)
constexpr size_t kPageableFetchBytes = 256u << 10;
struct FetchBlock {
  std::vector<uint32_t> pageable;
  std::optional<ImageLease> lease;
  uint32_t *p;
  FetchBlock(BufPool &pool, size_t words) {
    if (words * 4 <= kPageableFetchBytes) {
      pageable.resize(words);
      p = pageable.data();
    } else {
      lease.emplace(pool, words * 4);
      p = static_cast<uint32_t *>(lease->p);
    }
  }
};

// `words` words of a batch's side buffer whose last word is the error word (the arrays of a collapse, top_hits,
// composite or term bucket batch): ONE D2H copy (as slg_batch_fetch), waited for; rows a scoring wave gave up on
// are not made into an answer
struct SideBlock : FetchBlock {
  SideBlock(const slg_batch *b, const DevBuf &side, size_t words, hipStream_t st) : FetchBlock(b->idx->pool, words) {
    SLG_HIP(hipMemcpyAsync(p, side.p, words * 4, hipMemcpyDeviceToHost, st));
    SLG_HIP(wait_stream(st));
    if (p[words - 1] != 0u)
      throw SlgError(SLG_ERR_INTERNAL, "a scoring wave gave up on a round (chunk-loop guard): results are incomplete");
  }
};

// where a kernel that walks the candidates behind the select (top_hits, composite, term buckets) adds up a query's
// matched docs: nowhere when the sorted select or, in score order, agg_kernel has counted them
inline unsigned long long *post_select_matched(const slg_batch *b) {
  return (b->sorted || b->aggs) ? nullptr : b->d_matched.as<unsigned long long>();
}
// the cells of the aggregation spec in a query's rows (all 0 without one): what a composite's or a term bucket
// node's own cells lie behind
struct AggSpecCells {
  uint32_t count = 0, stats = 0, value = 0;
  uint64_t all() const { return (uint64_t)count + stats + value; }
};
inline AggSpecCells agg_spec_cells(const slg_batch *b) {
  return b->aggs ? AggSpecCells{b->agg_count_cells, b->agg_stats_cells, b->agg_value_cells} : AggSpecCells{};
}

// what the kernels that walk a query's candidate regions share (the two selects, agg_kernel): the slices of each
// query, their regions, and the tombstones and filters of the batch's state
template <typename P>
void fill_candidates(P &p, const slg_batch *b) {
  const IndexState &S = *b->snap;
  p.queries = b->d_queries;
  p.slice_seg = b->d_slice_seg;
  p.slice_cbeg = b->d_slice_cbeg.as<uint64_t>();
  p.slice_ccnt = b->d_slice_ccnt.as<uint32_t>();
  p.cand = b->d_cand.as<uint2>();
  p.segs = S.d_segs.as<slg::SegDev>();
  p.q_filter = b->d_q_filter.as<uint32_t>();
  p.reject_table = S.d_reject_table.as<const uint32_t *>();
  p.n_segs = (uint32_t)S.segs.size();
}

// what the launches of the two clause-filter kernels share (P: slg::BoolFilterParams, slg_clause.hpp): the
// slices, the candidates and the term groups' tables of a bool or phrase batch
template <typename P>
void fill_clause_filter(P &p, const slg_batch *b) {
  p.segs = b->snap->d_segs.template as<slg::SegDev>();
  p.sq = b->d_sq;
  p.slice_sq = b->d_slice_sq;
  p.queries = b->d_bool_desc.as<const slg::BoolQuery>();
  p.terms = reinterpret_cast<const slg::BoolTerm *>(b->d_bool_desc.as<unsigned char>() +
                                                    (size_t)b->nq * sizeof(slg::BoolQuery));
  p.cand = b->d_cand.as<uint2>();
  p.slice_cbeg = b->d_slice_cbeg.as<uint64_t>();
  p.slice_ccnt = b->d_slice_ccnt.as<uint32_t>();
  p.q_scored = b->d_q_scored.as<uint32_t>();
  p.n_slices = b->n_slices;
  p.n_segs = (uint32_t)b->snap->segs.size();
}

// slg_aggs.hip: the checks of a spec that need no index (throws); the spec against the batch's state, the
// tables' layout and the device buffers (throws; the batch is otherwise prepared); the launch behind the
// batch's select kernel
void agg_check_spec(const slg_agg_spec *aggs);
void agg_attach(slg_batch *b, const slg_agg_spec &aggs);
void agg_launch(slg_batch *b, hipStream_t st);
// slg_rescore.hip: the planned rescore table onto the device with the batch's detail arrays (throws; the batch
// is otherwise prepared); the launch behind the batch's last first-pass kernel
void rescore_attach(slg_batch *b, const slgplan::RescorePlan &rp);
void rescore_launch(slg_batch *b, hipStream_t st);
// slg_bool.hip: the planned clause tables onto the device (throws; the batch is otherwise prepared); the launch
// behind the batch's scoring kernel, in front of its select
void bool_attach(slg_batch *b, const slgplan::BoolPlan &bp);
void bool_launch(slg_batch *b, hipStream_t st);
// slg_phrase.hip: the same for a phrase batch, behind bool_attach; the launch in bool_launch's place
void phrase_attach(slg_batch *b, const slgplan::PhrasePlan &pp);
void phrase_launch(slg_batch *b, hipStream_t st);
// slg_booltree.hip: the planned tables of a tree batch onto the device; the launch in bool_launch's place
void booltree_attach(slg_batch *b, const slgplan::BoolTreePlan &tp);
void booltree_launch(slg_batch *b, hipStream_t st);
// slg_fscore.hip: an index state's aggregation columns as plan_fscore reads them; the planned tables onto the
// device (throws; the batch is otherwise prepared); the launch behind the batch's scoring kernel, in front of
// its select
std::vector<slgplan::FscoreFieldView> fscore_field_views(const IndexState &S);
void fscore_attach(slg_batch *b, const slgplan::FscorePlan &fp);
void fscore_launch(slg_batch *b, hipStream_t st);
// slg_script.hip: the same for the script stage of a script batch
void script_attach(slg_batch *b, const slgplan::ScriptPlan &sp, bool first);
void script_launch(slg_batch *b, hipStream_t st);
// slg_scan.hip: the launch of a scan batch's candidate source, in the place of the partition and scoring kernels
void scan_launch(slg_batch *b, hipStream_t st);
// slg_collapse.hip: the spec against the batch's state (its keyword column, the inner sort's columns), the tables
// and side arrays onto the device (throws; the batch is otherwise prepared); the launch behind the batch's rows
void collapse_attach(slg_batch *b, const slg_collapse_spec &spec, const slg_sort_spec *batch_sort);
void collapse_launch(slg_batch *b, hipStream_t st);
// slg_tophits.hip: the spec against the batch's state (the nodes' sort columns, the parents' rows), the tables,
// output arrays and run scratch onto the device (throws; the batch is otherwise prepared, agg_attach has run); the
// launch behind agg_kernel (without an aggregation spec: behind the select)
void top_hits_attach(slg_batch *b, const slg_top_hits_spec &spec);
void top_hits_launch(slg_batch *b, hipStream_t st);
// slg_composite.hip: the checks of a composite spec that need no index (throws; after agg_check_spec); the spec
// against the batch's state (the sources' columns and key layout, the children's tables), descriptors, ranks and
// tables onto the device (throws; the batch is otherwise prepared, agg_attach has run); the two launches behind
// agg_kernel (without an aggregation spec: behind the select)
void composite_check_spec(const slg_composite_spec *spec);
void composite_attach(slg_batch *b, const slg_composite_spec &spec);
void composite_launch(slg_batch *b, hipStream_t st);
// slg_aggs.hip: a composite's children planned as the roots of `size` parent rows, behind the composite's own count
// row and cells_before cells of the aggregation spec: the AggNodeDev and ColumnDev images, the layout (offsets into
// the composite's tables) and the cells of the composite's count and stats tables
struct CompositeChildTables {
  std::vector<unsigned char> nodes, cols;
  std::vector<slg_agg_layout> layout;
  uint64_t count_cells = 0, stats_cells = 0;
  bool ext = false;
};
CompositeChildTables agg_plan_children(const IndexState &S, const slg_composite_spec &spec, uint64_t cells_before);
// slg_termbuckets.hip: the checks of a term bucket spec that need no index (throws; after agg_check_spec); the spec
// against the batch's state (columns, filters, ranks, the background tables, the children's tables) onto the device
// (throws; the batch is otherwise prepared, agg_attach has run); the launches behind agg_kernel (without an
// aggregation spec: behind the select)
void term_buckets_check_spec(const slg_term_bucket_spec *spec);
void term_buckets_attach(slg_batch *b, const slg_term_bucket_spec &spec);
void term_buckets_launch(slg_batch *b, hipStream_t st);

// slg_vsearch.hip: one vector search or hybrid call, checked against one state of the index ...
struct VsCall {
  std::shared_ptr<const IndexState> S;
  uint32_t nq = 0, n_clauses = 0, cand = 0, k_out = 0;
  uint32_t dim[SLG_MAX_VECTOR_CLAUSES] = {}, coff[SLG_MAX_VECTOR_CLAUSES] = {};
  int32_t metric[SLG_MAX_VECTOR_CLAUSES] = {};
  const slg::VecSegDev *vsegs[SLG_MAX_VECTOR_CLAUSES] = {};
  const slg::VecCopyDev *csegs[SLG_MAX_VECTOR_CLAUSES] = {};  // (slg_vector_search_batch_approx*) the fields' bf16 copies
  const VecListField *lists[SLG_MAX_VECTOR_CLAUSES] = {};     // (slg_vector_search_batch_ivf*) the fields' lists
  uint32_t q_floats = 0;
};
// ... and its arrays (host or device memory, as the entry says)
struct VsArgs {
  const float *qvecs, *alpha, *boost;
  const int32_t *q_filter;
  uint32_t *out_doc, *out_seg;
  float *out_score, *out_vec;
  uint32_t *out_count;
  uint64_t *out_total;
};
// every check of such a call, before any device work.  false: nq == 0, nothing to do.  host_filter: q_filter is
// host memory and its ids are checked here.  state: the one to check against (null: the index's current one)
bool vs_prepare(slg_index *ix, uint32_t nq, uint32_t n_clauses, const uint32_t *clause_field, uint32_t cand_size,
                uint32_t k_out, const VsArgs &a, bool host_filter, VsCall *vc,
                std::shared_ptr<const IndexState> state = nullptr);
// slg_vsearch.hip: the bf16 copy of one store of n_rows x dim f32 values on the device (vs_quantize_kernel on the
// index stream, waited for); the caller holds the index's device
std::shared_ptr<VecCopySeg> vs_quantize_store(slg_index *ix, const float *d_values, uint32_t n_rows, uint32_t dim);
// slg_vsearch.hip: the lists of one store around n_lists host centroids (the assignment is an exact scan of the
// centroids with the store's rows as queries; count, scan and ordered fill on the index stream, waited for); the
// caller holds the index's device
std::shared_ptr<VecListSeg> vs_cluster_store(slg_index *ix, const uint32_t *d_offsets, const float *d_values,
                                             uint32_t n_docs, uint32_t n_rows, uint32_t dim, int32_t metric,
                                             const float *centroids, uint32_t n_lists);
// slg_vsearch.hip: at most iters Lloyd steps from init (null: rows of the store) on the index stream, then the
// lists of the final centroids (slg_index_train_vector_field); its scratch is gone when it returns
std::shared_ptr<VecListSeg> vs_train_store(slg_index *ix, const uint32_t *d_offsets, const float *d_values,
                                           uint32_t n_docs, uint32_t n_rows, uint32_t dim, int32_t metric,
                                           const float *init, uint32_t n_lists, uint32_t iters,
                                           slg_vector_train_stats *stats);
// slg_vsearch.hip: the steps a hybrid call (slg_hybrid.hip) shares with the vector search, whose kernels they
// run.  HyWork: the clause lists and sort space of one call, laid out over one block (base null: the size only);
// cnt = run_cnt [clause][nq] then key_cnt [clause][nq], zeroed by the caller
struct HyWork {
  uint64_t *run, *dlist, *ukeys, *bkeys;
  uint32_t *cnt;
  uint32_t P, Pb;
};
size_t hy_work_layout(const VsCall &vc, uint32_t bm_k, void *base, HyWork *w);
// the keys hy_gather_kernel appended for queries q_lo .. q_hi - 1: clause c's at keys + c * stride, query q's
// from q_cand[q] - slot_lo on; max_cap = the most slots a query of the range has
struct HyKeys {
  const uint64_t *keys;
  uint64_t stride, slot_lo, max_cap;
  const uint64_t *q_cand;
  uint32_t q_lo, q_hi;
};
void hy_fold(const VsCall &vc, const HyWork &w, const HyKeys &k, hipStream_t st);
// union with the BM25 rows [nq][bm_k], blend, top k_out
void hy_blend(const VsCall &vc, const VsArgs &a, const HyWork &w, const uint32_t *bm_doc, const uint32_t *bm_seg,
              const float *bm_score, const uint32_t *bm_count, uint32_t bm_k, hipStream_t st);
template <typename K, typename P>
void launch_kernel_lds(K kernel, const P &params, dim3 grid, uint32_t threads, size_t lds, hipStream_t st) {
  if (lds > 48 * 1024)
    SLG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
  hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, st, params);
  SLG_HIP(hipGetLastError());
}

// slg_rerank.hip: dimension / metric / device stores of vector field f (0: the field of the segment
// descriptors; mixed_metric: its segments may differ in metric — the single-clause kernel reads it per
// segment — and *metric is the last one's)
void field_facts(const IndexState &S, uint32_t f, uint32_t *dim, int32_t *metric, const slg::VecSegDev **vsegs,
                 bool mixed_metric = false);

}  // namespace slghost
