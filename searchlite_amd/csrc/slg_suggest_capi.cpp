// slg_suggest_capi.cpp — a small C ABI over the completion suggester's host side (slg_suggest_host.cpp) and over
// the per-candidate code of its kernels (slg_suggest.hpp, compiled for the host here) for the CPU unit tests
// (tests/test_suggest_ref.py), plus a straightforward restatement of the reference's loop
// (slgx_reference_suggest): what a caller without the device runs, and what tools/suggest_time.py times against.
// Built into lib/libslg_plan.so with g++; NOT part of libsearchlite_gpu.so's exported surface.
#include <algorithm>
#include <cstring>
#include <thread>
#include <unordered_map>

#include "slg_suggest_host.hpp"

bool ref_bounded_levenshtein(const std::vector<uint32_t> &a, const std::vector<uint32_t> &b, size_t max_edits, size_t *out);

namespace {
template <typename F>
int guarded(char *err, uint32_t err_len, F &&f) {
  try {
    f();
    return SLG_OK;
  } catch (const slgplan::SlgError &e) {
    if (err && err_len) {
      std::strncpy(err, e.what(), err_len - 1);
      err[err_len - 1] = 0;
    }
    return e.code;
  }
}

struct Option {
  uint32_t seg, pos;
  float score;
  uint64_t doc_freq;
};
struct SegRows {
  const uint32_t *pos;
  const uint8_t *dist;
  const uint32_t *df;
  uint32_t n;
};

// suggest_merge_kernel's five steps, one after the other, through the very functions the kernel calls
std::vector<Option> merge_one(const slgsuggest::Request &rq, const slgexpand::Dict *const *dicts, uint32_t n_segs,
                              const SegRows *rows) {
  struct Cand {
    uint32_t seg, pos, dist, df;
    const unsigned char *text;
    uint32_t len;
  };
  const uint32_t fb = (uint32_t)rq.field_key.size(), skip = (uint32_t)rq.range_key.size() - fb;
  std::vector<Cand> cands;
  for (uint32_t s = 0; s < n_segs && rq.scan; s++) {
    const uint32_t take = slg::suggest_take(std::min(rows[s].n, rq.cap), rq.cap, (uint32_t)cands.size());
    for (uint32_t i = 0; i < take; i++) {
      const std::string_view key = dicts[s]->key(rows[s].pos[i]);
      cands.push_back(Cand{s, rows[s].pos[i], rows[s].dist[i], rows[s].df[i],
                           reinterpret_cast<const unsigned char *>(key.data()) + fb, (uint32_t)key.size() - fb});
    }
  }
  std::vector<uint32_t> idx(cands.size());
  for (uint32_t i = 0; i < idx.size(); i++) idx[i] = i;
  const auto cmp = [&](uint32_t a, uint32_t b) {
    return slg::suggest_text_cmp(cands[a].text, cands[a].len, cands[b].text, cands[b].len, skip);
  };
  std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
    const int c = cmp(a, b);
    return c < 0 || (c == 0 && a < b);
  });
  std::vector<Option> groups;
  std::vector<uint64_t> keys;
  for (size_t k = 0; k < idx.size();) {
    float score = 0.0f;
    uint64_t df = 0;
    size_t m = k;
    do {
      const Cand &c = cands[idx[m]];
      score = slg::suggest_add(score, rq.fuzzy, c.dist, c.df);
      df += c.df;
      m++;
    } while (m < idx.size() && cmp(idx[m - 1], idx[m]) == 0);
    keys.push_back(slg::suggest_order_key(score, (uint32_t)groups.size()));
    groups.push_back(Option{cands[idx[k]].seg, cands[idx[k]].pos, score, df});
    k = m;
  }
  std::sort(keys.begin(), keys.end());
  std::vector<Option> out;
  for (size_t i = 0; i < keys.size() && i < rq.size; i++) out.push_back(groups[(size_t)(keys[i] & 0xFFFFFFFFull)]);
  return out;
}

// collect_completion_candidates + completion_suggest as the reference runs them (:1785-1877, :1941-1977)
struct RefOption {
  std::string text;
  float score;
  uint64_t doc_freq;
};
std::vector<RefOption> ref_suggest_one(const slgsuggest::Request &rq, const slgexpand::Dict *const *dicts,
                                       const uint32_t *const *dfs, uint32_t n_segs) {
  std::vector<RefOption> out;
  if (!rq.scan) return out;
  struct Acc {
    uint64_t doc_freq = 0;
    float score = 0.0f;
  };
  std::unordered_map<std::string, Acc> merged;
  const size_t fpl = rq.field_key.size();
  size_t expanded = 0;
  for (uint32_t s = 0; s < n_segs && expanded < rq.cap; s++) {
    uint32_t lo, hi;
    slgexpand::prefix_range(*dicts[s], rq.range_key, lo, hi);
    for (uint32_t p = lo; p < hi && expanded < rq.cap; p++) {
      const std::string_view key = dicts[s]->key(p);
      if (key.size() <= fpl) continue;
      const std::string_view cand = key.substr(fpl);
      float w = 1.0f;
      if (rq.fuzzy) {
        std::vector<uint32_t> cc;
        slgexpand::utf8_decode(cand.data(), cand.size(), &cc);
        const size_t cl = cc.size(), tl = rq.cps.size();
        if ((cl > tl ? cl - tl : tl - cl) > rq.max_edits) continue;
        size_t d;
        if (!ref_bounded_levenshtein(rq.cps, cc, rq.max_edits, &d)) continue;
        w = 1.0f / ((float)d + 1.0f);
      }
      const uint32_t df = dfs[s][p];
      if (df == 0) continue;
      Acc &a = merged[std::string(cand)];
      a.doc_freq += df;
      const float part = rq.fuzzy ? w * (float)df : (float)df;
      a.score = a.score + part;
      expanded++;
    }
  }
  for (auto &kv : merged) out.push_back(RefOption{kv.first, kv.second.score, kv.second.doc_freq});
  std::sort(out.begin(), out.end(), [](const RefOption &a, const RefOption &b) {
    return a.score != b.score ? a.score > b.score : a.text < b.text;
  });
  if (out.size() > rq.size) out.resize(rq.size);
  return out;
}
}  // namespace

extern "C" {

// the checks of a request; on success whether it scans, whether it is fuzzy, its cap, its clamped max_edits and
// its range key (range_cap bytes)
int slgx_suggest_check(const slg_suggest_req *r, uint32_t *scan, uint32_t *fuzzy, uint32_t *cap, uint32_t *max_edits,
                       char *range_key, uint32_t range_cap, uint32_t *range_len, char *err, uint32_t err_len) {
  return guarded(err, err_len, [&] {
    const slgsuggest::Request q = slgsuggest::check_request(*r, 0);
    *scan = q.scan;
    *fuzzy = q.fuzzy;
    *cap = q.cap;
    *max_edits = q.max_edits;
    *range_len = (uint32_t)q.range_key.size();
    std::memcpy(range_key, q.range_key.data(), std::min<size_t>(range_cap, q.range_key.size()));
  });
}

// what the scan owes the merge for one (request, segment), by the kernel's predicate on the host: the first
// min(cap, row_cap) passing keys of the (for a plain request: clipped) range; df [n] in sorted-position order.
// *total = the passing keys of the range that was scanned
int slgx_suggest_scan(const slg_suggest_req *r, const void *dict, const uint32_t *df, uint32_t row_cap, uint32_t *row_pos,
                      uint8_t *row_dist, uint32_t *row_df, uint32_t *n_rows, uint32_t *total, char *err, uint32_t err_len) {
  return guarded(err, err_len, [&] {
    const slgsuggest::Request q = slgsuggest::check_request(*r, 0);
    const auto &d = *static_cast<const slgexpand::Dict *>(dict);
    *n_rows = *total = 0;
    if (!q.scan) return;
    std::vector<uint32_t> nonzero((size_t)d.n() + 1, 0u);
    for (uint32_t p = 0; p < d.n(); p++) nonzero[p + 1] = nonzero[p] + (df[p] != 0u);
    uint32_t lo, hi;
    slgexpand::prefix_range(d, q.range_key, lo, hi);
    if (!q.fuzzy) hi = slgsuggest::clip_plain(nonzero, lo, hi, q.cap);
    const slg::SuggestReqDev rd = slgsuggest::device_request(q);
    const slg::SuggestSegDev sg{reinterpret_cast<const unsigned char *>(d.bytes.data()), d.offs.data(), d.nchars.data(), df};
    for (uint32_t p = lo; p < hi; p++) {
      uint32_t dist;
      if (!slg::suggest_pass(&rd, rd.cp, sg, p, dist)) continue;
      if (*total < q.cap && *total < row_cap) {
        row_pos[*n_rows] = p;
        row_dist[*n_rows] = (uint8_t)dist;
        row_df[*n_rows] = df[p];
        (*n_rows)++;
      }
      (*total)++;
    }
  });
}

// the merge over hand-made scan rows: segment s's rows are row_offsets[s] .. row_offsets[s + 1] - 1
int slgx_suggest_merge(const slg_suggest_req *r, const void *const *dicts, uint32_t n_segs, const uint32_t *row_offsets,
                       const uint32_t *row_pos, const uint8_t *row_dist, const uint32_t *row_df, uint32_t opt_cap,
                       uint32_t *out_seg, uint32_t *out_pos, float *out_score, uint64_t *out_doc_freq, uint32_t *n_opts,
                       char *err, uint32_t err_len) {
  return guarded(err, err_len, [&] {
    const slgsuggest::Request q = slgsuggest::check_request(*r, 0);
    std::vector<SegRows> rows(n_segs);
    for (uint32_t s = 0; s < n_segs; s++)
      rows[s] = SegRows{row_pos + row_offsets[s], row_dist + row_offsets[s], row_df + row_offsets[s], row_offsets[s + 1] - row_offsets[s]};
    const std::vector<Option> opts = merge_one(q, reinterpret_cast<const slgexpand::Dict *const *>(dicts), n_segs, rows.data());
    *n_opts = (uint32_t)opts.size();
    if (opts.size() > opt_cap) throw slgplan::SlgError(SLG_ERR_INVALID, "slgx_suggest_merge: opt_cap too small");
    for (size_t i = 0; i < opts.size(); i++) {
      out_seg[i] = opts[i].seg;
      out_pos[i] = opts[i].pos;
      out_score[i] = opts[i].score;
      out_doc_freq[i] = opts[i].doc_freq;
    }
  });
}

// The reference's loop on the host for n_reqs requests over n_threads threads (requests dealt round robin);
// dfs[s]: segment s's df in sorted-position order.  Output as slg_suggest_batch lays it out; the four arrays may
// all be NULL (timing: the options are counted only)
int slgx_reference_suggest(const void *const *dicts, const uint32_t *const *dfs, uint32_t n_segs, const slg_suggest_req *reqs,
                           uint32_t n_reqs, uint32_t n_threads, uint32_t *out_offsets, uint32_t option_capacity,
                           float *out_score, uint64_t *out_doc_freq, uint32_t *out_text_offsets, uint32_t text_capacity,
                           char *out_text, char *err, uint32_t err_len) {
  return guarded(err, err_len, [&] {
    std::vector<slgsuggest::Request> rq;
    for (uint32_t i = 0; i < n_reqs; i++) rq.push_back(slgsuggest::check_request(reqs[i], i));
    std::vector<std::vector<RefOption>> opts(n_reqs);
    const auto *dd = reinterpret_cast<const slgexpand::Dict *const *>(dicts);
    const auto work = [&](uint32_t t) {
      for (uint32_t i = t; i < n_reqs; i += n_threads) opts[i] = ref_suggest_one(rq[i], dd, dfs, n_segs);
    };
    n_threads = std::max(1u, n_threads);
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < n_threads; t++) pool.emplace_back(work, t);
    work(0);
    for (auto &th : pool) th.join();
    uint32_t at = 0, bytes = 0;
    for (uint32_t i = 0; i < n_reqs; i++) {
      out_offsets[i] = at;
      for (const RefOption &o : opts[i]) {
        if (out_score) {
          if (at >= option_capacity || bytes + o.text.size() > text_capacity)
            throw slgplan::SlgError(SLG_ERR_INVALID, "slgx_reference_suggest: a capacity is too small");
          out_score[at] = o.score;
          out_doc_freq[at] = o.doc_freq;
          out_text_offsets[at] = bytes;
          std::memcpy(out_text + bytes, o.text.data(), o.text.size());
        }
        at++;
        bytes += (uint32_t)o.text.size();
      }
    }
    out_offsets[n_reqs] = at;
    if (out_score) out_text_offsets[at] = bytes;
  });
}

}  // extern "C"
