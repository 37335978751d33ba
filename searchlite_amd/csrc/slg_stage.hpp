// slg_stage.hpp — the kernels that build what an index keeps on the device: per-posting impacts and
// per-term champion bounds at staging time (and again when live_docs changes), the reject bitmaps of
// doc filters.  Only slg_index.hip includes it (a static kernel is compiled into every unit that
// includes its header).  Wave-level helpers: slg_wave.hpp.
//
// Path restated (reference file:line relative to searchlite-core/src/):
//   stage_impacts   : query/bm25.rs:1-6 + query/wand.rs:77-84,269-286 evaluated once per
//                     posting at staging time with weight factored out
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slg_desc.hpp"
#include "slg_wave.hpp"

namespace slg {

// ---- staging: per-posting impact ---------------------------------------------------------
// impact = bm25(tf, df, doc_len, avgdl, docs, k1, b) exactly as score_tf computes `base`
// (query/wand.rs:279-285 -> query/bm25.rs:1-6); idf is computed on the host with libm
// logf (bm25.rs:2, f32::ln) and passed per term.
struct StageParams {
  uint64_t n_postings;
  uint32_t n_terms;
  uint32_t n_docs;
  const uint64_t *term_offsets;  // [V+1] (unpadded: positions in docs / tfs)
  const uint32_t *docs;          // [P] as uploaded; nullptr: docs_out already holds them (re-derivation)
  const uint32_t *tfs;           // [P]
  const float *term_idf;         // [V]
  const uint16_t *term_field;    // [V] or nullptr
  const float *const *field_doc_len;  // [F] device pointers (or nullptr entries)
  const float *field_avgdl;           // [F]
  float k1, b;
  uint32_t *docs_out;  // out, padded layout: posting i of term t -> i + kListPad * t
  float *imps;         // out, padded layout
};

static __global__ void __launch_bounds__(256) stage_impacts_kernel(StageParams p) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; i < p.n_postings; i += stride) {
    // term of posting i: last t with term_offsets[t] <= i
    uint32_t lo = 0, hi = p.n_terms;  // invariant: off[lo] <= i < off[hi]
    while (hi - lo > 1) {
      uint32_t mid = lo + ((hi - lo) >> 1);
      if (p.term_offsets[mid] <= i)
        lo = mid;
      else
        hi = mid;
    }
    uint32_t t = lo;
    float df = (float)(uint32_t)(p.term_offsets[t + 1] - p.term_offsets[t]);
    (void)df;
    uint32_t f = p.term_field ? p.term_field[t] : 0;
    float avgdl = p.field_avgdl[f];
    const float *lens = p.field_doc_len[f];
    const uint64_t at = i + (uint64_t)kListPad * t;
    // creation: the uploaded doc id, scattered into the padded layout below; re-derivation after a
    // tombstone update (slg_index_update_deleted): the doc id is read back from there
    uint32_t doc = p.docs ? p.docs[i] : p.docs_out[at];
    float tf = (float)p.tfs[i];
    // ScoredTerm::doc_len  query/wand.rs:77-84
    float dl = fmaxf(avgdl, 1.0f);
    if (lens && doc < p.n_docs) {
      float v = lens[doc];
      if (v > 0.0f) dl = v;
    }
    // score_tf  query/wand.rs:279-283
    float norm_len = dl > 0.0f ? dl : fmaxf(avgdl, tf);
    // bm25  query/bm25.rs:2-5 (idf precomputed)
    float idf = p.term_idf[t];
    float norm_dl = avgdl > 0.0f ? norm_len / avgdl : 1.0f;
    float denom = tf + p.k1 * (1.0f - p.b + p.b * norm_dl);
    if (p.docs) p.docs_out[at] = doc;
    p.imps[at] = idf * (tf * (p.k1 + 1.0f)) / fmaxf(denom, 1e-6f);
  }
}

// ---- staging: per-term champion impacts ------------------------------------------------------
// champ[t][r], r = 0..63 (descending): a value v such that at least r+1 postings of term t have
// impact >= v (0 where the list is shorter).  Lane l scans postings l, l+64, ... and keeps its 16
// largest; the 64 lane maxima, sorted, give ranks 1..64.  champ[t][64..67] bound ranks 128, 256,
// 512, 1024: every lane holds j values >= its own j-th largest, so all lanes together hold 64*j
// values >= the minimum over lanes of the j-th largest (j = 2, 4, 8, 16).  Not the exact order
// statistics, but valid lower bounds, which is all the threshold seed needs: a doc's total
// score is >= any one of its (non-negative) per-term contributions.
struct ChampParams {
  const uint64_t *term_offsets;  // [V+1] (unpadded)
  const float *imps;             // padded layout (SegDev)
  const uint32_t *docs;          // padded layout
  const uint32_t *deleted;       // bitmap words or nullptr: deleted docs never count (accept())
  float *champ;                  // [V * kChampions]
  uint32_t n_terms;
};

static __global__ void __launch_bounds__(256) stage_champions_kernel(ChampParams p) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const uint32_t n_waves = gridDim.x * kWavesPerBlock;
  for (uint32_t t = wave; t < p.n_terms; t += n_waves) {
    const uint64_t a = p.term_offsets[t] + (uint64_t)kListPad * t;
    const uint64_t b = a + (p.term_offsets[t + 1] - p.term_offsets[t]);
    float m[16];
#pragma unroll
    for (int r = 0; r < 16; r++) m[r] = 0.0f;
    for (uint64_t i0 = a; i0 < b; i0 += 64) {
      const uint64_t i = i0 + lane;
      float x = i < b ? p.imps[i] : 0.0f;
      if (p.deleted && i < b) {
        const uint32_t d = p.docs[i];
        if ((p.deleted[d >> 5] >> (d & 31)) & 1u) x = 0.0f;
      }
      if (__ballot(x > m[15]) == 0ull) continue;  // nobody improves: the common case
#pragma unroll
      for (int r = 15; r >= 1; r--) m[r] = x > m[r - 1] ? m[r - 1] : (x > m[r] ? x : m[r]);
      m[0] = x > m[0] ? x : m[0];
    }
    // bounds for ranks 128 .. 1024
    float lo[4] = {m[1], m[3], m[7], m[15]};
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) lo[j] = fminf(lo[j], __shfl_xor(lo[j], o, 64));
    }
    // bitonic sort of the 64 lane maxima, descending (lane 0 = largest)
    float v = m[0];
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
      for (int d = size >> 1; d > 0; d >>= 1) {
        const float o = __shfl_xor(v, d, 64);
        const bool up = ((lane & size) == 0) == ((lane & d) == 0);  // keep the larger one
        v = up ? fmaxf(v, o) : fminf(v, o);
      }
    }
    float *row = p.champ + (size_t)t * kChampions;
    row[lane] = v;
    if (lane < 4) row[kChampSorted + lane] = lane == 0 ? lo[0] : lane == 1 ? lo[1] : lane == 2 ? lo[2] : lo[3];
  }
}

// ---- doc filters (accept = !deleted && filter, api/reader.rs:3009-3018) -----------
// A filter is kept per segment as a REJECT bitmap (deleted | ~filter, bit d of word d/32) so the
// scoring kernels use it exactly like the tombstone bitmap.
struct FilterBuildParams {
  const uint32_t *deleted;  // or nullptr
  const uint32_t *pass;     // uploaded pass bitmap (words), or nullptr when built from a column
  const void *column;       // i64 / f64 column [n_docs], or nullptr
  double lo_f, hi_f;
  long long lo_i, hi_i;
  int column_kind;  // 0 none, 1 i64, 2 f64
  uint32_t n_docs;
  uint32_t *reject;  // out [ceil(n_docs/32)]
  int invert_pass;        // the pass bitmap marks the docs to REJECT (docs that hold a not-term)
  const uint32_t *pass2;  // a second pass bitmap, AND-ed (the request's own filter), or nullptr
};

// marks the docs of one posting list in a bitmap (slg_index_add_filter_terms: the matcher's not-terms)
struct PostingMarkParams {
  const uint32_t *docs;  // the list's first posting (padded layout: only [0, df) are read)
  uint32_t df;
  uint32_t n_docs;
  uint32_t *bitmap;      // [ceil(n_docs/32)] zeroed before the first list
};
static __global__ void __launch_bounds__(256) posting_mark_kernel(PostingMarkParams p) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.df) return;
  const uint32_t d = p.docs[i];
  if (d < p.n_docs) atomicOr(&p.bitmap[d >> 5], 1u << (d & 31u));
}

static __global__ void __launch_bounds__(256) filter_build_kernel(FilterBuildParams p) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;  // one doc per lane
  const uint32_t lane = threadIdx.x & 63;
  bool pass = false;
  if (d < p.n_docs) {
    if (p.column_kind == 1) {
      const long long v = static_cast<const long long *>(p.column)[d];
      pass = v >= p.lo_i && v <= p.hi_i;
    } else if (p.column_kind == 2) {
      const double v = static_cast<const double *>(p.column)[d];
      pass = v >= p.lo_f && v <= p.hi_f;  // NaN never passes (query/filters.rs numeric range)
    } else {
      pass = p.pass == nullptr || ((((p.pass[d >> 5] >> (d & 31)) & 1u) != 0u) != (p.invert_pass != 0));
      if (p.pass2 && !((p.pass2[d >> 5] >> (d & 31)) & 1u)) pass = false;
    }
    if (p.deleted && ((p.deleted[d >> 5] >> (d & 31)) & 1u)) pass = false;
  }
  const uint64_t rej = ~__ballot(pass);  // docs past n_docs are rejected too
  const uint32_t w = d >> 5;
  if ((lane & 31u) == 0 && (d < p.n_docs))
    p.reject[w] = lane == 0 ? (uint32_t)rej : (uint32_t)(rej >> 32);
}

// reject bitmap of a filter after new tombstones: out = a | b (b may be null: no tombstones)
struct BitmapOrParams {
  const uint32_t *a, *b;
  uint32_t *out;
  uint32_t n_words;
};
static __global__ void __launch_bounds__(256) bitmap_or_kernel(BitmapOrParams p) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < p.n_words) p.out[i] = p.a[i] | (p.b ? p.b[i] : 0u);
}

}  // namespace slg
