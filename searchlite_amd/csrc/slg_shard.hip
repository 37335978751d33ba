// slg_shard.hip — index sharding over RCCL: the run-time binding of the library, shard groups, sharded runs
// and their results.
#include "slg_host.hpp"

#include <dlfcn.h>

#include <condition_variable>

using namespace slghost;

// ---- index sharding over RCCL (api/reader.rs:2670-2778 with segment = shard) --------
// One process (or host thread) per GPU holds the segments of its shard; every rank scores the same
// query batch, ONE ncclAllGather exchanges the contiguous per-rank result blocks
// doc | seg | score | count ((3k+1) * Q * 4 bytes) over xGMI, and every rank merges the world's rows
// by (score desc, segment_ord asc, doc asc), segment_ord = rank * segs_per_rank + local segment
// (query/sort.rs:80-93).  RCCL is bound at run time (dlopen): a single-GPU user of the library does
// not need it, and inside a PyTorch process the librccl torch has loaded is the one used.
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

extern "C" {

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
    KeepLastError keep;
    delete g;
    return nullptr;
  }
  return g;
}

void slg_shard_group_destroy(slg_shard_group *g) {
  if (!g) return;
  if (g->comm) {
    DeviceScope on(g->idx->device);
    (void)hipDeviceSynchronize();
    try {
      (void)rccl().destroy(g->comm);
    } catch (...) {
    }
    if (g->coll_stream) (void)hipStreamDestroy(g->coll_stream);
  }
  delete g;
}

namespace {
// the kinds of batch that do not run sharded (slg_batch_run_sharded*, slg_batch_fetch_sharded)
void require_shardable(const slg_batch *b) {
  // (a cursor's segment_ord is index-global; the shard merge does not apply it)
  if (b->after) throw SlgError(SLG_ERR_UNSUPPORTED, "a cursor batch does not run sharded");
  if (b->hybrid) throw SlgError(SLG_ERR_UNSUPPORTED, "a hybrid batch does not run sharded");
  if (b->aggs) throw SlgError(SLG_ERR_UNSUPPORTED, "an aggregation batch does not run sharded");
  if (b->rescore) throw SlgError(SLG_ERR_UNSUPPORTED, "a rescore batch does not run sharded");
  if (b->phrase) throw SlgError(SLG_ERR_UNSUPPORTED, "a phrase batch does not run sharded");
  if (b->boolean) throw SlgError(SLG_ERR_UNSUPPORTED, "a bool batch does not run sharded");
  if (b->booltree) throw SlgError(SLG_ERR_UNSUPPORTED, "a tree batch does not run sharded");
  if (b->fscore) throw SlgError(SLG_ERR_UNSUPPORTED, "a function_score batch does not run sharded");
  if (b->script) throw SlgError(SLG_ERR_UNSUPPORTED, "a script_score batch does not run sharded");
  if (b->collapse) throw SlgError(SLG_ERR_UNSUPPORTED, "a collapse batch does not run sharded");
  if (b->top_hits) throw SlgError(SLG_ERR_UNSUPPORTED, "a top_hits batch does not run sharded");
  if (b->composite) throw SlgError(SLG_ERR_UNSUPPORTED, "a composite batch does not run sharded");
  if (b->term_buckets) throw SlgError(SLG_ERR_UNSUPPORTED, "a term bucket batch does not run sharded");
  if (b->scan) throw SlgError(SLG_ERR_UNSUPPORTED, "a scan batch does not run sharded");
}

int run_sharded_impl(slg_batch *b, slg_shard_group *g, bool have_seq, uint64_t seq, uint32_t *out_doc,
                     uint32_t *out_seg, float *out_score, uint32_t *out_count) {
  int rc = guarded([&] {
    SLG_REQUIRE_LIVE(b);
    SLG_REQUIRE(g != nullptr && g->idx == b->idx, "shard group is NULL or belongs to another index");
    SLG_REQUIRE(g->segs_per_rank >= b->snap->segs.size(), "the shard grew beyond the group's segs_per_rank");
    require_shardable(b);
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
    const ResultBlock R(b->nq, b->k);
    const size_t blk = R.words();  // words of one rank's block
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
      uint32_t *gb = b->d_gather.as<uint32_t>();
      if (b->k == 0) {
        SLG_HIP(hipMemsetAsync(m, 0, blk * 4, st));
      } else {
        slg::ShardMergeParams mp{};
        mp.doc = R.doc(gb);
        mp.seg = R.seg(gb);
        mp.score = R.score(gb);
        mp.count = R.count(gb);
        mp.out_doc = R.doc(m);
        mp.out_seg = R.seg(m);
        mp.out_score = R.score(m);
        mp.out_count = R.count(m);
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
      b->last_sharded = true;
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
    require_shardable(b);
    SLG_REQUIRE(b->nq == 0 || out_count != nullptr, "out_count is NULL");
    SLG_REQUIRE(b->nq == 0 || b->k == 0 || (out_doc && out_seg && out_score), "output array is NULL");
    if (b->nq == 0) return;
    SLG_REQUIRE(b->d_merged.p != nullptr, "slg_batch_run_sharded has not run on this batch");
    slg_index *ix = b->idx;
    DeviceGuard dg(ix->device);
    const hipStream_t st = locked_stream(b);
    const ResultBlock R(b->nq, b->k);
    ImageLease lease(ix->pool, R.words() * 4);  // pinned staging (see slg_batch_fetch)
    uint32_t *h = static_cast<uint32_t *>(lease.p);
    SLG_HIP(hipMemcpyAsync(h, b->d_merged.p, R.words() * 4, hipMemcpyDeviceToHost, st));
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
    R.unpack(h, out_doc, out_seg, out_score, out_count);
  });
}

int slg_batch_sharded_device_results(slg_batch *b, void **d_doc, void **d_seg, void **d_score, void **d_count) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    SLG_REQUIRE(b->d_merged.p != nullptr || b->nq == 0, "slg_batch_run_sharded has not run on this batch");
    const ResultBlock R(b->nq, b->k);
    uint32_t *m = b->d_merged.as<uint32_t>();
    if (d_doc) *d_doc = m;
    if (d_seg) *d_seg = m ? R.seg(m) : nullptr;
    if (d_score) *d_score = m ? R.score(m) : nullptr;
    if (d_count) *d_count = m ? R.count(m) : nullptr;
  });
}

}  // extern "C"
