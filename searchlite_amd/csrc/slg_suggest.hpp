// slg_suggest.hpp — the device side of slg_suggest_batch: the completion suggester's scan and its
// merge.
//
// Scan.  The geometry, the ballot ranking and the distance of slg_expand.hpp with the completion rules
// (api/reader.rs:1785-1877): a key passes when it is not the bare key "field:", its posting list is not empty and,
// for a fuzzy request, its char count is within max_edits of the term's and its distance is <= max_edits, 0
// INCLUDED.  Per (request, segment) the first R = cap passing keys of the range in dictionary order, as sorted
// position, distance and doc frequency: the cap counts visits, so no segment can contribute more.  Own kernels
// (suggest_count_kernel, suggest_emit_kernel); the expansion's are untouched.
//
// Merge (suggest_merge_kernel).  One workgroup per request, a thread per candidate:
//   1. takes: segment by segment min(rows, cap - taken so far), at most kSuggestMaxCandidates in all;
//   2. a bitonic sort in LDS of the candidates by (text bytes, candidate number): equal texts of several segments
//      come to lie side by side in segment order (skipped when one segment contributed: its rows are sorted);
//   3. the head of every run of equal texts adds the run up one candidate at a time, in segment order;
//   4. a bitonic sort of the groups by one integer key (score descending, text rank ascending);
//   5. the first min(size, groups) go out as (segment, sorted position, score, doc_freq).
//
// The per-candidate rules (caps, take, text order, the sum, the final key) and the predicate are plain C++ that
// also compiles for the host: the CPU tests run exactly this code (slg_suggest_capi.cpp).
#pragma once

#define SLG_EXPAND_NO_KERNELS  // the geometry, utf8_next and banded_distance; the expansion's kernels stay in their unit
#include "slg_expand.hpp"

namespace slg {

constexpr uint32_t kSuggestMaxCandidates = 256;  // MAX_SUGGEST_CANDIDATES
constexpr uint32_t kSuggestMinScan = 64;         // DEFAULT_SUGGEST_SCAN
constexpr uint32_t kSuggestMergeThreads = 256;   // a thread per candidate
constexpr uint32_t kSuggestNoCand = 0xFFFFu;     // the sort's padding: after every candidate

// :1793-1795
SLG_XHD uint32_t suggest_plain_cap(const uint32_t size) {
  const uint64_t c = (uint64_t)size * 5u;
  return c < kSuggestMinScan ? kSuggestMinScan : (c > kSuggestMaxCandidates ? kSuggestMaxCandidates : (uint32_t)c);
}
// :1840-1841
SLG_XHD uint32_t suggest_fuzzy_cap(const uint32_t max_expansions, const uint32_t size) {
  const uint32_t c = max_expansions < kSuggestMaxCandidates ? max_expansions : kSuggestMaxCandidates;
  return c > size ? c : size;
}
// what a segment with `rows` passing keys adds when `taken` visits are already counted (:1803, :1818, :1844, :1866)
SLG_XHD uint32_t suggest_take(const uint32_t rows, const uint32_t cap, const uint32_t taken) {
  const uint32_t left = cap > taken ? cap - taken : 0u;
  return rows < left ? rows : left;
}
// the byte order of two texts (String::cmp); both start with the same `skip` bytes (the scanned prefix)
SLG_XHD int suggest_text_cmp(const unsigned char *a, const uint32_t alen, const unsigned char *b, const uint32_t blen,
                             const uint32_t skip) {
  const uint32_t n = alen < blen ? alen : blen;
  for (uint32_t i = skip; i < n; i++)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return alen < blen ? -1 : (alen > blen ? 1 : 0);
}
// one candidate into its text's score: plain `score += df as f32` (:1816); fuzzy `score += distance_weight(d) *
// df as f32` (:1864, :977-979): a divide, a multiply, an add, each rounded to f32 on its own
SLG_XHD float suggest_add(const float score, const bool fuzzy, const uint32_t dist, const uint32_t df) {
  if (!fuzzy) return score + (float)df;
  const float w = 1.0f / ((float)dist + 1.0f);
  const float part = w * (float)df;
  return score + part;
}
// the groups' order as one integer, ascending: score descending (scores are finite and above 0, so their bits
// order as they do), then the text's rank ascending (:1969-1974)
SLG_XHD uint64_t suggest_order_key(const float score, const uint32_t text_rank) {
  union {
    float f;
    uint32_t u;
  } b;
  b.f = score;
  return ((uint64_t)(0xFFFFFFFFu - b.u) << 32) | text_rank;
}

// ---- what the host stages for one call --------------------------------------------------------------------
struct SuggestReqDev {
  uint32_t fuzzy;        // 0 plain, 1 fuzzy
  uint32_t max_edits;    // fuzzy: 1 or 2
  uint32_t n_chars;      // code points of the term
  uint32_t field_bytes;  // bytes of "field:"
  uint32_t field_chars;  // chars of "field:"
  uint32_t skip_bytes;   // bytes of the scanned prefix behind "field:": every candidate's text starts with them
  uint32_t cap;          // visits the reference counts, <= kSuggestMaxCandidates
  uint32_t size;
  uint32_t cp[kExpandMaxChars];
};
// (pairs and chunks: ExpandPairDev, as the expansion's scan lays them out; a request's pairs lie side by side in
// segment order, req_pair[r] .. req_pair[r + 1] - 1)
struct SuggestScanParams {
  const SuggestReqDev *reqs;
  const SuggestSegDev *segs;
  const ExpandPairDev *pairs;
  const uint32_t *chunk_pair;  // [n_chunks]
  uint64_t *ballots;           // [n_chunks * kExpandWaves * kExpandIters]
  uint32_t *slab_count;        // [n_chunks * kExpandWaves]
  uint32_t *row_pos;           // [total rows] sorted positions
  uint8_t *row_dist;           // [total rows]
  uint32_t *row_df;            // [total rows]
  uint32_t *pair_total;        // [n_pairs] keys of the range that passed
};
struct SuggestMergeParams {
  const SuggestReqDev *reqs;
  const SuggestSegDev *segs;
  const ExpandPairDev *pairs;
  const uint32_t *req_pair;  // [n_reqs + 1]
  const uint32_t *row_pos;
  const uint8_t *row_dist;
  const uint32_t *row_df;
  const uint32_t *pair_total;
  const uint32_t *opt_base;  // [n_reqs] the request's first option slot; it owns min(size, cap) of them
  uint32_t *opt_seg, *opt_pos;
  float *opt_score;
  uint64_t *opt_df;
  uint32_t *n_opts;          // [n_reqs]
};

// the completion predicate on the key at sorted position pos (inside the range); dist: its distance (fuzzy)
SLG_XHD bool suggest_pass(const SuggestReqDev *rq, const uint32_t *cp, const SuggestSegDev &sg, const uint32_t pos,
                          uint32_t &dist) {
  dist = 0;
  const uint32_t a = sg.offs[pos], bytes = sg.offs[pos + 1] - a;
  if (bytes <= rq->field_bytes) return false;  // the key "field:" itself (:1806, :1847)
  if (sg.df[pos] == 0u) return false;          // :1811, :1859
  if (!rq->fuzzy) return true;
  uint32_t kc = sg.nchars[pos];
  if (kc == 255u) kc = utf8_count(sg.bytes + a, bytes);
  const int m = (int)(kc - rq->field_chars), n = (int)rq->n_chars;
  const int diff = m > n ? m - n : n - m;
  if (diff > (int)rq->max_edits) return false;  // :1852
  dist = banded_distance(cp, n, sg.bytes + a + rq->field_bytes, m, rq->max_edits);
  return dist <= rq->max_edits;  // :1855 (0: the candidate is the term, and it counts)
}

#if defined(__HIPCC__)

struct SuggestWork {
  const SuggestReqDev *rq;
  SuggestSegDev sg;
  uint32_t pair, first_slab, n_slabs, slab, begin, hi, rows, row_base;
};

__device__ __forceinline__ SuggestWork suggest_prologue(const SuggestScanParams &p, uint32_t *s_cp) {
  SuggestWork w;
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

static __global__ __launch_bounds__(kExpandThreads) void suggest_count_kernel(const SuggestScanParams p) {
  __shared__ uint32_t s_cp[kExpandMaxChars];
  const SuggestWork w = suggest_prologue(p, s_cp);
  const uint32_t lane = threadIdx.x % kExpandWave;
  uint32_t count = 0;
  for (uint32_t it = 0; it < kExpandIters; it++) {
    const uint32_t pos = w.begin + it * kExpandWave + lane;
    uint32_t dist;
    const bool pass = pos < w.hi && suggest_pass(w.rq, s_cp, w.sg, pos, dist);
    const uint64_t m = __ballot(pass);
    if (lane == 0) p.ballots[(size_t)w.slab * kExpandIters + it] = m;
    count += (uint32_t)__popcll(m);
  }
  if (lane == 0) p.slab_count[w.slab] = count;
}

static __global__ __launch_bounds__(kExpandThreads) void suggest_emit_kernel(const SuggestScanParams p) {
  __shared__ uint32_t s_cp[kExpandMaxChars];
  const SuggestWork w = suggest_prologue(p, s_cp);
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
      if (w.rq->fuzzy) (void)suggest_pass(w.rq, s_cp, w.sg, pos, dist);
      p.row_pos[w.row_base + rank] = pos;
      p.row_dist[w.row_base + rank] = (uint8_t)dist;
      p.row_df[w.row_base + rank] = w.sg.df[pos];
    }
    rank0 += (uint32_t)__popcll(m);
  }
}

// a bitonic sort of s[0 .. n2) (n2 a power of two <= kSuggestMergeThreads) by `less`, every thread of the
// workgroup calling it
template <typename T, typename Less>
__device__ __forceinline__ void suggest_bitonic(T *s, const uint32_t n2, const Less less) {
  const uint32_t t = threadIdx.x;
  for (uint32_t k = 2; k <= n2; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      const uint32_t o = t ^ j;
      if (t < n2 && o > t) {
        const T a = s[t], b = s[o];
        const bool up = (t & k) == 0u;
        if (less(b, a) == up) {  // (keys are distinct: exactly one of less(a, b), less(b, a) holds)
          s[t] = b;
          s[o] = a;
        }
      }
      __syncthreads();
    }
}

static __global__ __launch_bounds__(kSuggestMergeThreads) void suggest_merge_kernel(const SuggestMergeParams p) {
  constexpr uint32_t N = kSuggestMaxCandidates;
  static_assert(kSuggestMergeThreads == N, "a thread per candidate");
  __shared__ const unsigned char *s_text[N];  // candidate -> its text in its segment's dictionary
  __shared__ uint32_t s_len[N], s_seg[N], s_pos[N], s_df[N];
  __shared__ uint8_t s_dist[N], s_head[N];
  __shared__ uint16_t s_idx[N];               // text order -> candidate
  __shared__ uint64_t s_key[N], s_gdf[N];     // group -> order key, doc_freq
  __shared__ float s_gscore[N];
  __shared__ uint16_t s_gcand[N];             // group -> its first candidate
  __shared__ uint32_t s_wave[kSuggestMergeThreads / 64];
  const uint32_t r = blockIdx.x, t = threadIdx.x;
  const SuggestReqDev *rq = p.reqs + r;
  const uint32_t cap = rq->cap < N ? rq->cap : N, skip = rq->skip_bytes;
  const bool fuzzy = rq->fuzzy != 0u;

  // 1. the takes, segment by segment; candidate t is row t - taken of the pair that covers it
  uint32_t n = 0, contributors = 0;
  for (uint32_t pi = p.req_pair[r]; pi < p.req_pair[r + 1] && n < cap; pi++) {
    const ExpandPairDev pr = p.pairs[pi];
    const uint32_t total = p.pair_total[pi];
    const uint32_t take = suggest_take(total < pr.rows ? total : pr.rows, cap, n);
    if (t >= n && t < n + take) {
      const uint32_t row = pr.row_base + (t - n), pos = p.row_pos[row];
      const SuggestSegDev sg = p.segs[pr.seg];
      const uint32_t a = sg.offs[pos];
      s_text[t] = sg.bytes + a + rq->field_bytes;
      s_len[t] = sg.offs[pos + 1] - a - rq->field_bytes;
      s_seg[t] = pr.seg;
      s_pos[t] = pos;
      s_df[t] = p.row_df[row];
      s_dist[t] = p.row_dist[row];
    }
    contributors += take != 0u;
    n += take;
  }
  if (n == 0u) {  // (the same for every thread)
    if (t == 0u) p.n_opts[r] = 0u;
    return;
  }
  s_idx[t] = t < n ? (uint16_t)t : (uint16_t)kSuggestNoCand;
  __syncthreads();

  // 2. equal texts side by side, in segment order
  const auto same_text = [&](const uint32_t a, const uint32_t b) {
    return suggest_text_cmp(s_text[a], s_len[a], s_text[b], s_len[b], skip) == 0;
  };
  if (contributors > 1u) {
    uint32_t n2 = 1;
    while (n2 < n) n2 <<= 1;
    suggest_bitonic(s_idx, n2, [&](const uint16_t a, const uint16_t b) {
      if (a == kSuggestNoCand || b == kSuggestNoCand) return a != kSuggestNoCand;
      const int c = suggest_text_cmp(s_text[a], s_len[a], s_text[b], s_len[b], skip);
      return c < 0 || (c == 0 && a < b);
    });
  }

  // 3. the groups: a head where the text changes; its rank among the heads is the text's rank
  const bool head = t < n && (t == 0u || contributors == 1u || !same_text(s_idx[t - 1], s_idx[t]));
  s_head[t] = head ? 1 : 0;
  const uint64_t hm = __ballot(head);
  if (t % 64u == 0u) s_wave[t / 64u] = (uint32_t)__popcll(hm);
  __syncthreads();
  uint32_t gid = (uint32_t)__popcll(hm & ((1ull << (t % 64u)) - 1ull)), n_groups = 0;
  for (uint32_t w = 0; w < kSuggestMergeThreads / 64; w++) {
    gid += w < t / 64u ? s_wave[w] : 0u;
    n_groups += s_wave[w];
  }
  s_key[t] = ~0ull;  // (padding of the second sort: behind every group)
  if (head) {
    float score = 0.0f;
    uint64_t df = 0;
    uint32_t m = t;
    do {  // one candidate at a time, in segment order: no tree
      const uint32_t c = s_idx[m];
      score = suggest_add(score, fuzzy, s_dist[c], s_df[c]);
      df += s_df[c];
      m++;
    } while (m < n && !s_head[m]);
    s_gscore[gid] = score;
    s_gdf[gid] = df;
    s_gcand[gid] = s_idx[t];
  }
  __syncthreads();
  if (head) s_key[gid] = suggest_order_key(s_gscore[gid], gid);
  __syncthreads();

  // 4. score descending, text ascending
  if (n_groups > 1u) {
    uint32_t g2 = 1;
    while (g2 < n_groups) g2 <<= 1;
    suggest_bitonic(s_key, g2, [](const uint64_t a, const uint64_t b) { return a < b; });
  }

  // 5. the winners
  const uint32_t n_out = rq->size < n_groups ? rq->size : n_groups;
  if (t < n_out) {
    const uint32_t g = (uint32_t)(s_key[t] & 0xFFFFFFFFull), c = s_gcand[g], o = p.opt_base[r] + t;
    p.opt_seg[o] = s_seg[c];
    p.opt_pos[o] = s_pos[c];
    p.opt_score[o] = s_gscore[g];
    p.opt_df[o] = s_gdf[g];
  }
  if (t == 0u) p.n_opts[r] = n_out;
}

#endif  // __HIPCC__

}  // namespace slg
