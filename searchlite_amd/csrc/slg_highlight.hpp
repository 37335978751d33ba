// slg_highlight.hpp — the device side of slg_highlight_batch / slg_batch_highlight: the fragments
// of index/highlight.rs over the texts of slg_index_add_text_field, with the tags inserted.
//
// The reference builds one regex per (hit, field) — `\bw1\W+w2...\b` for every phrase, then `\bterm\b` for every
// term, joined by `|`, case-insensitive, leftmost-first — and runs it over the stored text.  For ASCII texts and
// words of [0-9A-Za-z_] a match is exactly a maximal run of word bytes that equals a term under ASCII case folding,
// and a phrase match exactly as many consecutive runs with anything that is no word byte between them; at a run
// start the phrases are tried in order, then the terms in order, and the first that matches decides where the match
// ends.  hl_match_at is that rule; everything else here finds run starts and moves bytes.
//
// Geometry.  One wave per item (query, hit, field spec), kHlWaves items of one (query, field spec) per workgroup:
// the workgroup stages the spec's word table, folded to lower case by the host, in LDS once.  hl_find_next walks a
// region of the text in tiles of 64 lanes x 16 bytes (aligned 16-byte loads; the doc starts at any byte), each lane
// turns its bytes into a word mask, run starts are word & ~(word << 1 | carry), a lane tries its run starts in
// order and the wave takes the lowest lane that matched by ballot.  The count pass (hl_count_kernel) finds the
// up to nf matches of the text, scans each fragment as a string of its own and records where it starts and how
// long it gets with its tags; hl_scan_kernel turns the per-item counts into offsets; the emit pass
// (hl_emit_kernel) scans each fragment again and writes it.  No floating point, no atomics, nothing depends on
// timing: every output position follows from the counts.
//
// hl_is_word, hl_match_at and hl_next_match are plain C++ that also compiles for the host: the sequential
// highlighter of slg_highlight_host.cpp and the CPU tests run exactly this code.
#pragma once

#include <stdint.h>

#include "slg_desc.hpp"  // TextSegDev: a segment's texts on the device

#ifndef SLG_XHD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SLG_XHD __host__ __device__ __forceinline__
#define SLG_XUNROLL _Pragma("unroll")
#else
#define SLG_XHD inline
#define SLG_XUNROLL
#endif
#endif

namespace slg {

constexpr uint32_t kHlMaxTerms = 32, kHlMaxPhrases = 8, kHlMaxPhraseWords = 8;
constexpr uint32_t kHlMaxWordBytes = 128, kHlMaxTag = 64, kHlMaxFragment = 1024, kHlMaxFragments = 8;
constexpr uint32_t kHlMaxWords = kHlMaxTerms + kHlMaxPhrases * kHlMaxPhraseWords;
constexpr uint32_t kHlThreads = 256, kHlWaves = 4;
constexpr uint32_t kHlLaneBytes = 16, kHlTile = 64 * kHlLaneBytes;
constexpr uint32_t kHlNone = 0xFFFFFFFFu;
constexpr uint32_t kHlScanThreads = 1024;
// statuses of an item: the three of the ABI, and what a row at or past a batch's count[q] has on the device (the
// host drops those rows)
constexpr uint8_t kHlOk = 0, kHlHost = 1, kHlNoText = 2, kHlNoRow = 0xFF;

// The word table of one field spec as the kernels read it from LDS (and the host highlighter from memory): the
// phrases' words first, phrase p's being words phrase_first[p] .. phrase_first[p + 1] - 1, then the terms, words
// phrase_first[n_phrases] .. n_words - 1.  Bytes are lower case.
struct HlTable {
  uint32_t len_mask[5];  // HlSpecDev::len_mask
  uint16_t word_off[kHlMaxWords + 1];
  uint8_t phrase_first[kHlMaxPhrases + 1];
  uint8_t bytes[kHlMaxWords * kHlMaxWordBytes];
};
// One field spec of one query.  Its table lies packed in the call's blob at `blob`: u16 word_off[n_words + 1], u8
// phrase_first[n_phrases + 1], the word bytes, pre_tag, post_tag
struct HlSpecDev {
  const TextSegDev *segs;  // the text field's table of the index state, [n_segs]
  uint32_t n_segs;
  uint32_t n_terms, n_phrases, n_words;
  uint32_t word_bytes;     // bytes of all words
  uint32_t fs, nf;         // fragment_size, number_of_fragments
  uint32_t pre_len, post_len;
  uint32_t blob;           // byte offset of the table in the blob (a multiple of 4)
  uint32_t len_mask[5];    // bit L: a term or a phrase's first word has L bytes (1 .. kHlMaxWordBytes)
  uint32_t pad_;
};
struct HlBlockDev {  // one workgroup: rows first_row .. first_row + kHlWaves - 1 of query q under spec `spec`
  uint32_t q, spec, first_row;
};
struct HlParams {
  const HlSpecDev *specs;
  const uint8_t *blob;
  const HlBlockDev *blocks;
  const uint32_t *q_spec;   // [nq + 1] a query's specs
  const uint32_t *q_slot;   // [nq] its first item slot; slot = q_slot[q] + row * n_specs(q) + (spec - q_spec[q])
  const uint32_t *q_hit;    // [nq] its first row in hit_seg / hit_doc
  const uint32_t *q_rows;   // [nq] its rows
  const uint32_t *hit_seg, *hit_doc;
  const uint32_t *count;    // [nq] rows at or past count[q] yield nothing; or nullptr: every row counts
  // per item slot, written by the count pass
  uint8_t *status;
  uint32_t *n_frags;
  uint32_t *item_bytes;
  uint32_t *frag_start;     // [slots * kHlMaxFragments] first text byte of the fragment
  uint32_t *frag_len;       // [slots * kHlMaxFragments] bytes of the finished string
  // hl_scan_kernel: exclusive sums over the slots, the totals at [n_slots]
  uint32_t n_slots;
  uint32_t *slot_frag0;     // [n_slots + 1]
  uint64_t *slot_text0;     // [n_slots + 1]
  // the emit pass
  uint32_t *out_text_offsets;  // [frag_cap]
  uint8_t *out_text;           // [text_cap]
  uint32_t frag_cap;
  uint64_t text_cap;
};

SLG_XHD bool hl_is_word(const uint8_t c) {
  return (uint8_t)(c - '0') < 10u || (uint8_t)((c | 0x20u) - 'a') < 26u || c == '_';
}
SLG_XHD uint8_t hl_fold(const uint8_t c) { return (uint8_t)(c - 'A') < 26u ? (uint8_t)(c + 32u) : c; }
// bytes of the run of word bytes that starts at p, inside [p, hi); kHlMaxWordBytes + 1: longer than any word
SLG_XHD uint32_t hl_run_len(const uint8_t *text, const uint32_t p, const uint32_t hi) {
  uint32_t n = 0;
  while (p + n < hi && n <= kHlMaxWordBytes && hl_is_word(text[p + n])) n++;
  return n;
}
SLG_XHD bool hl_word_eq(const uint8_t *text, const uint8_t *w, const uint32_t n) {
  for (uint32_t i = 0; i < n; i++)
    if (hl_fold(text[i]) != w[i]) return false;
  return true;
}
// The match that starts at the run start p of a string that ends at hi: its end, or 0 (a match is never empty, so
// no match ends at 0).  The phrases in order, then the terms in order; the first that matches wins.
SLG_XHD uint32_t hl_match_at(const HlTable &t, const uint32_t n_phrases, const uint32_t n_words,
                             const uint8_t *text, const uint32_t p, const uint32_t hi) {
  const uint32_t rl = hl_run_len(text, p, hi);
  if (rl > kHlMaxWordBytes || !((t.len_mask[rl >> 5] >> (rl & 31u)) & 1u)) return 0u;
  for (uint32_t ph = 0; ph < n_phrases; ph++) {
    const uint32_t w0 = t.phrase_first[ph], w1 = t.phrase_first[ph + 1];
    uint32_t q = p, r = rl;
    bool ok = true;
    for (uint32_t w = w0; w < w1; w++) {
      const uint32_t wl = (uint32_t)t.word_off[w + 1] - t.word_off[w];
      if (w > w0) {  // \W+ : q stands behind a run, so at least one byte is skipped or the string ends
        while (q < hi && !hl_is_word(text[q])) q++;
        if (q == hi) {
          ok = false;
          break;
        }
        r = hl_run_len(text, q, hi);
      }
      if (r != wl || !hl_word_eq(text + q, t.bytes + t.word_off[w], wl)) {
        ok = false;
        break;
      }
      q += wl;
    }
    if (ok) return q;
  }
  for (uint32_t w = t.phrase_first[n_phrases]; w < n_words; w++)
    if ((uint32_t)t.word_off[w + 1] - t.word_off[w] == rl && hl_word_eq(text + p, t.bytes + t.word_off[w], rl)) return p + rl;
  return 0u;
}
// The first match of the string text[lo .. hi) that starts at or after `from`, one byte at a time: its start (its
// end in mend), or kHlNone.  What hl_find_next computes with a wave
SLG_XHD uint32_t hl_next_match(const HlTable &t, const uint32_t n_phrases, const uint32_t n_words,
                               const uint8_t *text, const uint32_t lo, const uint32_t hi, const uint32_t from, uint32_t &mend) {
  for (uint32_t p = from; p < hi; p++) {
    if (!hl_is_word(text[p]) || (p > lo && hl_is_word(text[p - 1]))) continue;
    const uint32_t e = hl_match_at(t, n_phrases, n_words, text, p, hi);
    if (e) {
      mend = e;
      return p;
    }
  }
  return kHlNone;
}
// a fragment of the match that starts at ms in a text of len bytes (highlight.rs: start = m.start - min(m.start,
// fs / 2), end = min(len, start + fs))
SLG_XHD uint32_t hl_fragment_start(const uint32_t ms, const uint32_t fs) { return ms - (ms < fs / 2u ? ms : fs / 2u); }
SLG_XHD uint32_t hl_fragment_end(const uint32_t start, const uint32_t fs, const uint32_t len) {
  return len - start < fs ? len : start + fs;
}

#if defined(__HIPCC__) && !defined(SLG_HL_NO_KERNELS)

__device__ __forceinline__ uint32_t hl_rfl(const uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// hl_next_match by one wave; every argument and the result are the same in every lane.  The loads are aligned
// 16-byte loads at or after the 16-byte line that holds text[from] and in front of text + hi: inside the store,
// whose first byte is 16-byte aligned and which is padded by 16 bytes
__device__ __forceinline__ uint32_t hl_find_next(const HlTable &t, const uint32_t n_phrases, const uint32_t n_words,
                                                 const uint8_t *text, const uint32_t lo,
                                                 const uint32_t hi, const uint32_t from, const uint32_t lane, uint32_t &mend) {
  if (from >= hi) return kHlNone;
  const uintptr_t tbase = (uintptr_t)text, end = tbase + hi;
  for (uintptr_t a = (tbase + from) & ~(uintptr_t)(kHlLaneBytes - 1u); a < end; a += kHlTile) {
    const uintptr_t ca = a + (uintptr_t)kHlLaneBytes * lane;
    const int64_t rel = (int64_t)ca - (int64_t)tbase;  // the text offset of the lane's first byte: -15 or more
    uint32_t word = 0u;
    if (ca < end) {
      const uint4 v = *reinterpret_cast<const uint4 *>(ca);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      SLG_XUNROLL
      for (uint32_t b = 0; b < kHlLaneBytes; b++) {
        const int64_t pos = rel + b;
        const uint8_t c = (uint8_t)(w[b >> 2] >> ((b & 3u) * 8u));
        if (pos >= (int64_t)lo && pos < (int64_t)hi && hl_is_word(c)) word |= 1u << b;
      }
    }
    // the byte in front of the lane's first: a word byte of the string?
    const uint32_t carry = (ca < end && rel - 1 >= (int64_t)lo && hl_is_word(text[rel - 1])) ? 1u : 0u;
    uint32_t starts = word & ~((word << 1) | carry);
    const int64_t skip = (int64_t)from - rel;  // bits in front of `from`
    if (skip > 0) starts = skip >= (int64_t)kHlLaneBytes ? 0u : (starts & ~((1u << skip) - 1u));
    uint32_t ms = 0u, me = 0u;
    while (starts && !me) {
      const uint32_t b = (uint32_t)__builtin_ctz(starts);
      starts &= starts - 1u;
      ms = (uint32_t)(rel + b);
      me = hl_match_at(t, n_phrases, n_words, text, ms, hi);
    }
    const uint64_t won = __ballot(me != 0u);
    if (won) {
      const int first = __builtin_ctzll(won);
      mend = (uint32_t)__shfl((int)me, first, 64);
      return (uint32_t)__shfl((int)ms, first, 64);
    }
  }
  return kHlNone;
}

// the spec's table into LDS, by the whole workgroup
__device__ __forceinline__ void hl_stage_table(HlTable &t, const HlSpecDev &sp, const HlSpecDev *in_memory, const uint8_t *blob) {
  const uint8_t *src = blob + sp.blob;
  if (threadIdx.x < 5u) t.len_mask[threadIdx.x] = in_memory->len_mask[threadIdx.x];  // (indexed in memory, not in registers)
  const uint16_t *woff = reinterpret_cast<const uint16_t *>(src);
  for (uint32_t i = threadIdx.x; i <= sp.n_words; i += kHlThreads) t.word_off[i] = woff[i];
  const uint8_t *pf = src + 2u * (sp.n_words + 1u);
  for (uint32_t i = threadIdx.x; i <= sp.n_phrases; i += kHlThreads) t.phrase_first[i] = pf[i];
  const uint8_t *wb = pf + sp.n_phrases + 1u;
  for (uint32_t i = threadIdx.x; i < sp.word_bytes; i += kHlThreads) t.bytes[i] = wb[i];
  __syncthreads();
}

// the item of this wave: its slot, its text (null: none to scan) and the status the text decides
struct HlItem {
  uint32_t slot;
  const uint8_t *text;
  uint32_t len;
  uint8_t status;
};
__device__ __forceinline__ bool hl_item(const HlParams &p, const HlBlockDev &blk, const HlSpecDev &sp, const uint32_t wave, HlItem &it) {
  const uint32_t q = blk.q, row = blk.first_row + wave;
  if (row >= p.q_rows[q]) return false;
  const uint32_t n_specs = p.q_spec[q + 1] - p.q_spec[q];
  it.slot = p.q_slot[q] + row * n_specs + (blk.spec - p.q_spec[q]);
  it.text = nullptr;
  it.len = 0u;
  if (p.count && row >= p.count[q]) {
    it.status = kHlNoRow;
    return true;
  }
  const uint32_t seg = hl_rfl(p.hit_seg[p.q_hit[q] + row]), doc = hl_rfl(p.hit_doc[p.q_hit[q] + row]);
  it.status = kHlNoText;
  if (seg >= sp.n_segs) return true;
  const TextSegDev sg = sp.segs[seg];
  if (!sg.bytes || doc >= sg.n_docs) return true;
  it.status = kHlHost;
  if ((sg.non_ascii[doc >> 5] >> (doc & 31u)) & 1u) return true;
  it.status = kHlOk;
  const uint64_t a = sg.offs[doc], e = sg.offs[doc + 1];
  it.text = sg.bytes + a;
  it.len = hl_rfl((uint32_t)(e - a));
  return true;
}

__global__ void __launch_bounds__(kHlThreads) hl_count_kernel(const HlParams p) {
  __shared__ HlTable t;
  const HlBlockDev blk = p.blocks[blockIdx.x];
  const HlSpecDev sp = p.specs[blk.spec];
  hl_stage_table(t, sp, p.specs + blk.spec, p.blob);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  HlItem it;
  if (!hl_item(p, blk, sp, wave, it)) return;
  uint32_t n = 0u, bytes = 0u;
  if (it.text && it.len && sp.n_words) {
    uint32_t offset = 0u;
    while (n < sp.nf) {
      uint32_t me = 0u;
      const uint32_t ms = hl_find_next(t, sp.n_phrases, sp.n_words, it.text, 0u, it.len, offset, lane, me);
      if (ms == kHlNone) break;
      const uint32_t start = hl_fragment_start(ms, sp.fs), end = hl_fragment_end(start, sp.fs, it.len);
      uint32_t matches = 0u, pos = start, fe = 0u;
      while (hl_find_next(t, sp.n_phrases, sp.n_words, it.text, start, end, pos, lane, fe) != kHlNone) {
        matches++;
        pos = fe;
      }
      const uint32_t out = (end - start) + matches * (sp.pre_len + sp.post_len);
      if (lane == 0u) {
        p.frag_start[(size_t)it.slot * kHlMaxFragments + n] = start;
        p.frag_len[(size_t)it.slot * kHlMaxFragments + n] = out;
      }
      bytes += out;
      n++;
      offset = me;
    }
  }
  if (lane == 0u) {
    p.status[it.slot] = it.status;
    p.n_frags[it.slot] = n;
    p.item_bytes[it.slot] = bytes;
  }
}

// exclusive sums of n_frags and item_bytes over the slots by ONE workgroup: a thread sums a contiguous share, the
// shares are scanned in LDS, the thread writes its share's prefixes
__global__ void __launch_bounds__(kHlScanThreads) hl_scan_kernel(const HlParams p) {
  __shared__ uint64_t s_text[kHlScanThreads];
  __shared__ uint32_t s_frag[kHlScanThreads];
  const uint32_t tid = threadIdx.x, per = (p.n_slots + kHlScanThreads - 1u) / kHlScanThreads;
  const uint32_t a = tid * per < p.n_slots ? tid * per : p.n_slots, e = a + per < p.n_slots ? a + per : p.n_slots;
  uint64_t text = 0u;
  uint32_t frags = 0u;
  for (uint32_t i = a; i < e; i++) {
    text += p.item_bytes[i];
    frags += p.n_frags[i];
  }
  s_text[tid] = text;
  s_frag[tid] = frags;
  __syncthreads();
  for (uint32_t o = 1u; o < kHlScanThreads; o <<= 1) {
    const uint64_t ut = tid >= o ? s_text[tid - o] : 0u;
    const uint32_t uf = tid >= o ? s_frag[tid - o] : 0u;
    __syncthreads();
    s_text[tid] += ut;
    s_frag[tid] += uf;
    __syncthreads();
  }
  uint64_t t0 = s_text[tid] - text;
  uint32_t f0 = s_frag[tid] - frags;
  for (uint32_t i = a; i < e; i++) {
    p.slot_text0[i] = t0;
    p.slot_frag0[i] = f0;
    t0 += p.item_bytes[i];
    f0 += p.n_frags[i];
  }
  if (tid == kHlScanThreads - 1u) {
    p.slot_text0[p.n_slots] = s_text[tid];
    p.slot_frag0[p.n_slots] = s_frag[tid];
  }
}

// n bytes from src to out_text[at ..) by the wave; nothing is written at or past text_cap
__device__ __forceinline__ void hl_copy(const HlParams &p, const uint64_t at, const uint8_t *src, const uint32_t n, const uint32_t lane) {
  for (uint32_t i = lane; i < n; i += 64u)
    if (at + i < p.text_cap) p.out_text[at + i] = src[i];
}

__global__ void __launch_bounds__(kHlThreads) hl_emit_kernel(const HlParams p) {
  __shared__ HlTable t;
  const HlBlockDev blk = p.blocks[blockIdx.x];
  const HlSpecDev sp = p.specs[blk.spec];
  hl_stage_table(t, sp, p.specs + blk.spec, p.blob);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  HlItem it;
  if (!hl_item(p, blk, sp, wave, it)) return;
  const uint32_t n = p.n_frags[it.slot];
  if (!it.text || n == 0u) return;
  const uint8_t *pre = p.blob + sp.blob + 2u * (sp.n_words + 1u) + sp.n_phrases + 1u + sp.word_bytes, *post = pre + sp.pre_len;
  const uint32_t f0 = p.slot_frag0[it.slot];
  uint64_t at = p.slot_text0[it.slot];
  for (uint32_t j = 0; j < n && j < kHlMaxFragments; j++) {
    const uint32_t start = hl_rfl(p.frag_start[(size_t)it.slot * kHlMaxFragments + j]);
    const uint32_t out = hl_rfl(p.frag_len[(size_t)it.slot * kHlMaxFragments + j]);
    if (start > it.len) break;  // (never: the count pass wrote it from this text)
    const uint32_t end = hl_fragment_end(start, sp.fs, it.len);
    if (lane == 0u && f0 + j < p.frag_cap) p.out_text_offsets[f0 + j] = (uint32_t)at;
    uint64_t w = at;
    uint32_t pos = start, me = 0u;
    for (;;) {
      const uint32_t ms = hl_find_next(t, sp.n_phrases, sp.n_words, it.text, start, end, pos, lane, me);
      if (ms == kHlNone) break;
      hl_copy(p, w, it.text + pos, ms - pos, lane);
      w += ms - pos;
      hl_copy(p, w, pre, sp.pre_len, lane);
      w += sp.pre_len;
      hl_copy(p, w, it.text + ms, me - ms, lane);
      w += me - ms;
      hl_copy(p, w, post, sp.post_len, lane);
      w += sp.post_len;
      pos = me;
    }
    hl_copy(p, w, it.text + pos, end - pos, lane);
    at += out;
  }
}

#endif  // __HIPCC__ && !SLG_HL_NO_KERNELS

}  // namespace slg
