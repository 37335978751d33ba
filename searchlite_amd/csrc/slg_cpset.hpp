// slg_cpset.hpp — the bounded per-wave key set of the selections that keep the `size` smallest u64 keys of a query:
// composite_select_kernel (slg_composite.hpp: the packed tuples of the candidates) and term_bucket_select_kernel
// (slg_termbuckets.hpp: the packed rows of a dense count table).  How it is used and why it is exact: the head of
// slg_composite.hpp.  Device code only, no kernel: both units include it without compiling the other's kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slg_aggs.hpp"

namespace slg {

constexpr uint32_t kCpThreads = kAggThreads;
constexpr uint32_t kCpWaves = kCpThreads / 64;
constexpr uint32_t kCpMaxSize = 1024;    // SLG_MAX_COMPOSITE_SIZE
constexpr uint32_t kCpMinCap = 512;      // entries of the smallest per-wave set: a step adds up to 64 keys to a set
                                         // at its fill limit, and a slot must stay empty for the probes to end
constexpr uint32_t kCpKeep = (kCpMaxSize + 1 + 63) / 64;  // keys a lane holds across a compaction
constexpr unsigned long long kCpEmpty = ~0ull;            // (key_bits <= 63: no key)

// entries of one wave's set for a request of `size` buckets; its fill limit
__host__ __device__ inline uint32_t cp_cap(const uint32_t size) {
  uint32_t cap = kCpMinCap;
  while (cap < 2u * (size + 1u)) cap <<= 1;
  return cap;
}
__host__ __device__ inline uint32_t cp_fill_limit(const uint32_t cap) { return cap - cap / 4u; }

// LDS traffic of one wave on its own region: what a lane wrote is what another lane of the wave reads next
__device__ __forceinline__ void cp_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// One wave's bounded set (see the head of the file).  Every method runs for all lanes of the wave together.
struct CpSet {
  unsigned long long *H;
  uint32_t cap, size, count;
  unsigned long long T;
  __device__ __forceinline__ void clear(const uint32_t lane) {
    for (uint32_t i = lane; i < cap; i += 64) H[i] = kCpEmpty;
    cp_wave_sync();
  }
  __device__ __forceinline__ uint32_t home(const unsigned long long key) const {
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32) & (cap - 1u);
  }
  // true: the key was not in the set (at least one slot is always empty, so the probe ends)
  __device__ __forceinline__ bool insert(const unsigned long long key) {
    uint32_t h = home(key);
    for (;;) {
      const unsigned long long old = atomicCAS(&H[h], kCpEmpty, key);
      if (old == kCpEmpty) return true;
      if (old == key) return false;
      h = (h + 1u) & (cap - 1u);
    }
  }
  // ascending, the empty slots last
  __device__ __forceinline__ void sort(const uint32_t lane) {
    cp_wave_sync();
    for (uint32_t k = 2; k <= cap; k <<= 1) {
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        for (uint32_t t = lane; t < cap / 2u; t += 64) {
          const uint32_t lo = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), hi = lo | j;
          const unsigned long long x = H[lo], y = H[hi];
          if ((x > y) == ((lo & k) == 0u)) {
            H[lo] = y;
            H[hi] = x;
          }
        }
        cp_wave_sync();
      }
    }
  }
  // sorted; the size + 1 smallest stay, T falls to just above the largest of them
  __device__ __forceinline__ void compact(const uint32_t lane) {
    sort(lane);
    const uint32_t keep = count < size + 1u ? count : size + 1u;
    if (count > size) T = H[size] + 1ull;
    unsigned long long R[kCpKeep];
#pragma unroll
    for (uint32_t j = 0; j < kCpKeep; j++) R[j] = j * 64u + lane < keep ? H[j * 64u + lane] : kCpEmpty;
    cp_wave_sync();
    clear(lane);
#pragma unroll
    for (uint32_t j = 0; j < kCpKeep; j++)
      if (R[j] != kCpEmpty) insert(R[j]);
    cp_wave_sync();
    count = keep;
  }
  __device__ __forceinline__ void offer(const bool has, const unsigned long long key, const uint32_t lane) {
    const bool fresh = has && key < T && insert(key);
    count += (uint32_t)__popcll(__ballot(fresh));
    if (count > cp_fill_limit(cap)) compact(lane);
  }
};

}  // namespace slg
