// slg_expand.hpp — the scan of slg_expand_batch: for every (request, segment) the first R keys of the request's
// range of the segment's sorted dictionary that pass the request's predicate, in dictionary order, as sorted
// positions plus edit distance, and the number that passed.
//
// Shape.  A range is cut into chunks of kExpandChunk keys; a workgroup of kExpandThreads threads takes one chunk,
// each of its waves a slab of kExpandSlab consecutive keys, 64 at a time, a lane per candidate key.  All waves of
// a workgroup serve one request, so its code points sit in LDS once and the predicate's parameters are
// wave-uniform.  Two kernels, no hand-off between workgroups inside either:
//   expand_count_kernel  evaluates the predicate: one ballot per 64 keys and one count per slab;
//   expand_emit_kernel   sums the counts of the slabs in front of its own (the rank of its first passing key),
//                        leaves if they already hold R rows (the reference's `break`), else ranks its passing
//                        keys from the ballots and writes those below R; only they get their distance computed
//                        a second time.
// Order comes from ballots and prefix counts alone: no atomics, the same rows on every run.
//
// The predicates (utf8_next, banded_distance, glob_match) are plain C++ and also compile for the host: the CPU
// tests run exactly this code against the reference's restatement (slg_expand_capi.cpp).
#pragma once

#include <stdint.h>

#include "slg_desc.hpp"  // ExpandSegDev: a segment's dictionary on the device

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SLG_XHD __host__ __device__ __forceinline__
#define SLG_XUNROLL _Pragma("unroll")
#else
#define SLG_XHD inline
#define SLG_XUNROLL
#endif

namespace slg {

constexpr uint32_t kExpandWave = 64;
constexpr uint32_t kExpandThreads = 256;
constexpr uint32_t kExpandChunk = 1024;
constexpr uint32_t kExpandWaves = kExpandThreads / kExpandWave;
constexpr uint32_t kExpandSlab = kExpandChunk / kExpandWaves;  // keys of one wave
constexpr uint32_t kExpandIters = kExpandSlab / kExpandWave;   // ballots of one slab
constexpr uint32_t kExpandMaxChars = 128;
constexpr int32_t kExpandFuzzy = 0, kExpandPrefix = 1, kExpandWildcard = 2;
constexpr uint32_t kExpandNoDistance = 1000;  // "no bounded distance": above any sum the band can hold

// the UTF-8 scalar value at p and its length in bytes.  The bytes are valid UTF-8 (dictionary keys and request
// strings are checked on the host before they reach this), so a lead byte's continuation bytes exist
SLG_XHD uint32_t utf8_next(const unsigned char *p, uint32_t &len) {
  const uint32_t b0 = p[0];
  if (b0 < 0x80u) {
    len = 1;
    return b0;
  }
  if (b0 < 0xE0u) {
    len = 2;
    return ((b0 & 0x1Fu) << 6) | (p[1] & 0x3Fu);
  }
  if (b0 < 0xF0u) {
    len = 3;
    return ((b0 & 0x0Fu) << 12) | ((p[1] & 0x3Fu) << 6) | (p[2] & 0x3Fu);
  }
  len = 4;
  return ((b0 & 0x07u) << 18) | ((p[1] & 0x3Fu) << 12) | ((p[2] & 0x3Fu) << 6) | (p[3] & 0x3Fu);
}

SLG_XHD uint32_t utf8_count(const unsigned char *p, uint32_t bytes) {
  uint32_t n = 0;
  for (uint32_t i = 0; i < bytes; i++) n += (p[i] & 0xC0u) != 0x80u;
  return n;
}

// bounded_levenshtein (api/reader.rs:981-1018) for max_edits <= 2 between the term's code points t[0 .. n) and
// a candidate of m chars in UTF-8 at c, |n - m| <= 2: the distance if it is <= max_edits, else
// kExpandNoDistance.  Only cells with |i - j| <= 2 can hold a value <= 2, and a path that leaves that band
// costs more than 2, so five cells per row, in registers, give every answer <= 2 exactly: cell d of row i is
// column j = i + d - 2 (rows: chars of the candidate, decoded as they come; columns: chars of the term).
// The reference's early exit on a row's minimum is kept: row minima never decrease, so it changes no answer
// and lets a wave whose lanes all fail leave early.
SLG_XHD uint32_t banded_distance(const uint32_t *t, const int n, const unsigned char *c, const int m,
                                 const uint32_t max_edits) {
  constexpr uint32_t INF = kExpandNoDistance;
  uint32_t prev[5], cur[5];
  SLG_XUNROLL
  for (int d = 0; d < 5; d++) prev[d] = (d >= 2 && d - 2 <= n) ? (uint32_t)(d - 2) : INF;
  uint32_t off = 0;
  for (int i = 1; i <= m; i++) {
    uint32_t len;
    const uint32_t ch = utf8_next(c + off, len);
    off += len;
    uint32_t row_min = INF;
  SLG_XUNROLL
    for (int d = 0; d < 5; d++) {
      const int j = i + d - 2;
      uint32_t v = INF;
      if (j == 0) {
        v = (uint32_t)i;
      } else if (j > 0 && j <= n) {
        v = prev[d] + (ch != t[j - 1] ? 1u : 0u);                  // substitute
        if (d < 4) v = prev[d + 1] + 1u < v ? prev[d + 1] + 1u : v;  // row i - 1, same column
        if (d > 0) v = cur[d - 1] + 1u < v ? cur[d - 1] + 1u : v;    // row i, column j - 1
      }
      cur[d] = v;
      row_min = v < row_min ? v : row_min;
    }
    if (row_min > max_edits) return INF;
  SLG_XUNROLL
    for (int d = 0; d < 5; d++) prev[d] = cur[d];
  }
  const int last = n - m + 2;  // the cell of column n in row m
  uint32_t res = INF;
  SLG_XUNROLL
  for (int d = 0; d < 5; d++) res = d == last ? prev[d] : res;
  return res <= max_edits ? res : INF;
}

// build_wildcard_regex (api/reader.rs:1216-1230) without a regex engine: the whole text (UTF-8, `bytes` long)
// against pat[0 .. n) where '*' is any run of chars and '?' one char, neither U+000A, anything else literal.
// The iterative two-pointer match: remember the last '*' and where its run ends, and on a mismatch let it take
// one more char.  Exact for this language: a '*' that would have to take U+000A fails the match, because that
// char can only pair with a literal of the pattern and no earlier '*' can reach across one either.
SLG_XHD bool glob_match(const uint32_t *pat, const uint32_t n, const unsigned char *text, const uint32_t bytes) {
  uint32_t p = 0, t = 0, star_p = 0xFFFFFFFFu, star_t = 0;
  while (t < bytes) {
    uint32_t len;
    const uint32_t ch = utf8_next(text + t, len);
    if (p < n && pat[p] == (uint32_t)'*') {
      star_p = p++;
      star_t = t;
      continue;
    }
    if (p < n && (pat[p] == (uint32_t)'?' ? ch != 0x0Au : pat[p] == ch)) {
      p++;
      t += len;
      continue;
    }
    if (star_p == 0xFFFFFFFFu) return false;
    const uint32_t taken = utf8_next(text + star_t, len);
    if (taken == 0x0Au) return false;
    star_t += len;
    t = star_t;
    p = star_p + 1;
  }
  while (p < n && pat[p] == (uint32_t)'*') p++;
  return p == n;
}

// ---- what the host stages for one call --------------------------------------------------------------------
struct ExpandReqDev {
  int32_t kind;
  uint32_t max_edits;    // fuzzy: 1 or 2
  uint32_t n_chars;      // code points of the term / pattern
  uint32_t field_bytes;  // bytes of "field:" — every key of a range starts with them
  uint32_t field_chars;  // chars of "field:"
  uint32_t cp[kExpandMaxChars];
};
// one (request, segment) with a non-empty range [lo, hi) of sorted positions: its first `rows` passing keys go
// to row_base ..; its chunks are first_chunk .. in the chunk table
struct ExpandPairDev {
  uint32_t req, seg, lo, hi, rows, row_base, first_chunk, pad;
};
struct ExpandParams {
  const ExpandReqDev *reqs;
  const ExpandSegDev *segs;
  const ExpandPairDev *pairs;
  const uint32_t *chunk_pair;  // [n_chunks]
  uint64_t *ballots;           // [n_chunks * kExpandWaves * kExpandIters]
  uint32_t *slab_count;        // [n_chunks * kExpandWaves]
  uint32_t *row_pos;           // [total rows] sorted positions
  uint8_t *row_dist;           // [total rows]
  uint32_t *pair_total;        // [n_pairs] keys of the range that passed
};

#if defined(__HIPCC__) && !defined(SLG_EXPAND_NO_KERNELS)  // (slg_suggest.hpp takes the pieces above, not the kernels)

// the request's predicate on the key at sorted position pos (inside the range); dist: its distance (fuzzy)
__device__ __forceinline__ bool expand_pass(const ExpandReqDev *rq, const uint32_t *cp, const ExpandSegDev &sg,
                                            const uint32_t pos, uint32_t &dist) {
  dist = 0;
  const uint32_t a = sg.offs[pos], bytes = sg.offs[pos + 1] - a;
  if (bytes <= rq->field_bytes) return false;  // the key "field:" itself
  if (rq->kind == kExpandPrefix) return true;
  const unsigned char *cand = sg.bytes + a + rq->field_bytes;
  if (rq->kind == kExpandWildcard) return glob_match(cp, rq->n_chars, cand, bytes - rq->field_bytes);
  // fuzzy: the char counts reject most keys before any key byte is read
  uint32_t kc = sg.nchars[pos];
  if (kc == 255u) kc = utf8_count(sg.bytes + a, bytes);
  const int m = (int)(kc - rq->field_chars), n = (int)rq->n_chars;
  const int diff = m > n ? m - n : n - m;
  if (diff > (int)rq->max_edits) return false;
  dist = banded_distance(cp, n, cand, m, rq->max_edits);
  return dist >= 1u && dist <= rq->max_edits;  // (0: the candidate is the term)
}

struct ExpandWork {
  const ExpandReqDev *rq;
  ExpandSegDev sg;
  uint32_t pair, first_slab, n_slabs, slab, begin, hi, rows, row_base;
};

// what both kernels start with: the chunk's pair, the request's code points into LDS, the wave's slab
__device__ __forceinline__ ExpandWork expand_prologue(const ExpandParams &p, uint32_t *s_cp) {
  ExpandWork w;
  const uint32_t chunk = blockIdx.x;
  w.pair = p.chunk_pair[chunk];
  const ExpandPairDev pr = p.pairs[w.pair];
  w.rq = p.reqs + pr.req;
  w.sg = p.segs[pr.seg];
  const uint32_t n_chars = w.rq->n_chars < kExpandMaxChars ? w.rq->n_chars : kExpandMaxChars;
  for (uint32_t i = threadIdx.x; i < n_chars; i += kExpandThreads) s_cp[i] = w.rq->cp[i];
  __syncthreads();
  const uint32_t wave = threadIdx.x / kExpandWave;
  w.first_slab = pr.first_chunk * kExpandWaves;
  w.n_slabs = ((pr.hi - pr.lo + kExpandChunk - 1) / kExpandChunk) * kExpandWaves;
  w.slab = chunk * kExpandWaves + wave;
  w.begin = pr.lo + (chunk - pr.first_chunk) * kExpandChunk + wave * kExpandSlab;
  w.hi = pr.hi;
  w.rows = pr.rows;
  w.row_base = pr.row_base;
  return w;
}

static __global__ __launch_bounds__(kExpandThreads) void expand_count_kernel(const ExpandParams p) {
  __shared__ uint32_t s_cp[kExpandMaxChars];
  const ExpandWork w = expand_prologue(p, s_cp);
  const uint32_t lane = threadIdx.x % kExpandWave;
  uint32_t count = 0;
  for (uint32_t it = 0; it < kExpandIters; it++) {
    const uint32_t pos = w.begin + it * kExpandWave + lane;
    uint32_t dist;
    const bool pass = pos < w.hi && expand_pass(w.rq, s_cp, w.sg, pos, dist);
    const uint64_t m = __ballot(pass);
    if (lane == 0) p.ballots[(size_t)w.slab * kExpandIters + it] = m;
    count += (uint32_t)__popcll(m);
  }
  if (lane == 0) p.slab_count[w.slab] = count;
}

static __global__ __launch_bounds__(kExpandThreads) void expand_emit_kernel(const ExpandParams p) {
  __shared__ uint32_t s_cp[kExpandMaxChars];
  const ExpandWork w = expand_prologue(p, s_cp);
  const uint32_t lane = threadIdx.x % kExpandWave;
  uint32_t part = 0;
  for (uint32_t s = w.first_slab + lane; s < w.slab; s += kExpandWave) part += p.slab_count[s];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
  uint32_t rank0 = part;  // passing keys of the range in front of this slab
  if (w.slab == w.first_slab + w.n_slabs - 1 && lane == 0) p.pair_total[w.pair] = rank0 + p.slab_count[w.slab];
  for (uint32_t it = 0; it < kExpandIters && rank0 < w.rows; it++) {
    const uint64_t m = p.ballots[(size_t)w.slab * kExpandIters + it];
    const uint32_t rank = rank0 + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (((m >> lane) & 1ull) && rank < w.rows) {
      const uint32_t pos = w.begin + it * kExpandWave + lane;
      uint32_t dist = 0;
      if (w.rq->kind == kExpandFuzzy) (void)expand_pass(w.rq, s_cp, w.sg, pos, dist);
      p.row_pos[w.row_base + rank] = pos;
      p.row_dist[w.row_base + rank] = (uint8_t)dist;
    }
    rank0 += (uint32_t)__popcll(m);
  }
}

#endif  // __HIPCC__ && !SLG_EXPAND_NO_KERNELS

}  // namespace slg
