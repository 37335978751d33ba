// slg_expand_regex.hpp — the regex predicate of slg_expand_batch's scan: a lane walks one key's term bytes through
// the request's byte-level DFA (slg_regex.hpp compiles it on the host), and expand_regex_count_kernel, which does
// for regex requests what expand_count_kernel (slg_expand.hpp) does for the other kinds: the same geometry, the
// same ballots and slab counts, so expand_emit_kernel serves both.  DESIGN.md 5p "Regex".
//
// A request's DFA travels as one blob: 256 bytes of byte -> class, then n_states x n_classes bytes of transitions
// (state-major; state 0 dead, state 1 start), padded to a multiple of 4, then 32 bytes of accept bits.  The
// kernel copies map and table into LDS once per workgroup, a dword per thread and step; the accept bits are read
// once per key from global memory.
//
// LDS layout.  Both reads of a step are byte reads at lane-divergent addresses; the banks are dwords, lanes that
// read the same dword are served together, and the conflict groups are the two 32-lane halves.  State-major
// keeps a state's row in n_classes consecutive bytes: keys of one range share prefixes and most patterns hold
// most lanes in a few states, so the lanes of a half read a few short rows, and a row of up to 128 classes lies
// on distinct banks.  The map is 64 dwords: bytes b and b + 128 share a bank, so ASCII terms read it without a
// conflict.  That is reasoning from the bank rule; the conflict rate is NOT measured.
#pragma once

#include "slg_expand.hpp"

namespace slg {

constexpr int32_t kExpandRegex = 4;
constexpr uint32_t kRegexMaxStates = 256, kRegexMaxTable = 16384, kRegexAcceptBytes = 32;

// where a request's DFA lies in the blob array (bytes, a multiple of 4); n_states == 0: not a regex request
struct RegexReqDev {
  uint32_t blob_off, n_states, n_classes, table_bytes;  // table_bytes: n_states x n_classes rounded up to 4
};

// one step of the walk
SLG_XHD uint32_t regex_step(const uint8_t *class_of, const uint8_t *table, const uint32_t n_classes, const uint32_t state,
                            const uint32_t byte) {
  return table[state * n_classes + class_of[byte]];
}
SLG_XHD bool regex_accepts(const uint8_t *accept, const uint32_t state) { return (accept[state >> 3] >> (state & 7u)) & 1u; }

#if defined(__HIP_DEVICE_COMPILE__)
#define SLG_REGEX_ANY(x) (__any(x) != 0)  // the wave goes on while one of its lanes does
#else
#define SLG_REGEX_ANY(x) (x)
#endif

// the whole text (`bytes` long) through the DFA: stops on the dead state; true if the last state accepts.  On the
// device every lane of the wave calls this together (a lane without a key with bytes == 0)
SLG_XHD bool regex_walk(const uint8_t *class_of, const uint8_t *table, const uint8_t *accept, const uint32_t n_classes,
                        const unsigned char *text, const uint32_t bytes) {
  uint32_t state = 1;
  for (uint32_t i = 0;; i++) {
    const bool go = i < bytes && state != 0u;
    if (!SLG_REGEX_ANY(go)) break;
    if (go) state = regex_step(class_of, table, n_classes, state, text[i]);
  }
  return regex_accepts(accept, state);
}

struct ExpandRegexParams {
  ExpandParams p;
  const RegexReqDev *rx;   // [n_reqs]
  const uint8_t *blobs;
  uint32_t chunk_base;     // the first regex chunk of the chunk table: block b scans chunk chunk_base + b
};

#if defined(__HIPCC__) && !defined(SLG_EXPAND_NO_KERNELS)

static __global__ __launch_bounds__(kExpandThreads) void expand_regex_count_kernel(const ExpandRegexParams q) {
  __shared__ __attribute__((aligned(16))) uint8_t s_class[256];
  __shared__ __attribute__((aligned(16))) uint8_t s_table[kRegexMaxTable];
  const ExpandParams &p = q.p;
  const uint32_t chunk = q.chunk_base + blockIdx.x;
  const ExpandPairDev pr = p.pairs[p.chunk_pair[chunk]];
  const ExpandReqDev *rq = p.reqs + pr.req;
  const RegexReqDev rx = q.rx[pr.req];
  const ExpandSegDev sg = p.segs[pr.seg];
  const uint8_t *blob = q.blobs + rx.blob_off;
  {  // map and table into LDS, a dword at a time (blob_off and table_bytes are multiples of 4; both are clamped
     // to the arrays here whatever the host staged)
    const uint32_t *src = reinterpret_cast<const uint32_t *>(blob);
    uint32_t *dc = reinterpret_cast<uint32_t *>(s_class), *dt = reinterpret_cast<uint32_t *>(s_table);
    if (threadIdx.x < 64u) dc[threadIdx.x] = src[threadIdx.x];
    const uint32_t words = (rx.table_bytes < kRegexMaxTable ? rx.table_bytes : kRegexMaxTable) / 4u;
    for (uint32_t i = threadIdx.x; i < words; i += kExpandThreads) dt[i] = src[64u + i];
  }
  __syncthreads();
  const uint8_t *accept = blob + 256u + rx.table_bytes;
  const uint32_t wave = threadIdx.x / kExpandWave, lane = threadIdx.x % kExpandWave;
  const uint32_t slab = chunk * kExpandWaves + wave;
  const uint32_t begin = pr.lo + (chunk - pr.first_chunk) * kExpandChunk + wave * kExpandSlab;
  uint32_t count = 0;
  for (uint32_t it = 0; it < kExpandIters; it++) {
    const uint32_t pos = begin + it * kExpandWave + lane;
    uint32_t a = 0, bytes = 0;
    if (pos < pr.hi) {
      a = sg.offs[pos];
      bytes = sg.offs[pos + 1] - a;
    }
    const bool has_term = bytes > rq->field_bytes;  // (not the key "field:" itself, not a lane past the range)
    const bool match = regex_walk(s_class, s_table, accept, rx.n_classes, sg.bytes + a + rq->field_bytes,
                                  has_term ? bytes - rq->field_bytes : 0u);
    const uint64_t m = __ballot(has_term && match);
    if (lane == 0) p.ballots[(size_t)slab * kExpandIters + it] = m;
    count += (uint32_t)__popcll(m);
  }
  if (lane == 0) p.slab_count[slab] = count;
}

#endif  // __HIPCC__ && !SLG_EXPAND_NO_KERNELS

}  // namespace slg
