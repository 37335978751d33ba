// slg_expand_capi.cpp — a small C ABI over the host side of term expansion (slg_expand_merge.cpp) and over the
// scan's predicates (slg_expand.hpp, compiled for the host here) for the CPU unit tests (tests/test_expand_ref.py),
// plus a straightforward restatement of the reference's expansion loop (slgx_reference_expand): what a caller
// without the device scan runs, and what tools/expand_time.py times it against.  Built into lib/libslg_plan.so
// with g++; NOT part of libsearchlite_gpu.so's exported surface.
#include <cstring>
#include <thread>
#include <unordered_set>

#include "slg_expand.hpp"
#include "slg_expand_merge.hpp"
#include "slg_expand_regex.hpp"

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

}  // namespace

// bounded_levenshtein, api/reader.rs:981-1018, over code points: two full rows, the row-minimum exit
// (slg_suggest_capi.cpp's restatement of the reference's suggest loop calls it too: external linkage)
bool ref_bounded_levenshtein(const std::vector<uint32_t> &a, const std::vector<uint32_t> &b, size_t max_edits, size_t *out) {
  const size_t a_len = a.size(), b_len = b.size();
  if ((a_len > b_len ? a_len - b_len : b_len - a_len) > max_edits) return false;
  if (a_len == 0 || b_len == 0) {
    *out = a_len + b_len;
    return *out <= max_edits;
  }
  std::vector<size_t> prev(b_len + 1), curr(b_len + 1, 0);
  for (size_t j = 0; j <= b_len; j++) prev[j] = j;
  for (size_t i = 0; i < a_len; i++) {
    curr[0] = i + 1;
    size_t row_min = curr[0];
    for (size_t j = 0; j < b_len; j++) {
      const size_t cost = a[i] == b[j] ? 0 : 1;
      const size_t val = std::min(std::min(prev[j + 1] + 1, curr[j] + 1), prev[j] + cost);
      curr[j + 1] = val;
      row_min = std::min(row_min, val);
    }
    if (row_min > max_edits) return false;
    std::swap(prev, curr);
  }
  *out = prev[b_len];
  return *out <= max_edits;
}

namespace {

// expand_term_fuzzy / expand_prefix / expand_wildcard / expand_regex as the reference runs them: walk the range of every
// segment, test every key, keep a set of the keys seen
void ref_expand_one(const slgexpand::Request &rq, const slgexpand::Dict *const *dicts, uint32_t n_segs,
                    std::vector<uint32_t> &ids, std::vector<uint8_t> &dist) {
  using namespace slgexpand;
  const auto emit = [&](const std::string &key, uint8_t d) {
    for (uint32_t t = 0; t < n_segs; t++) {
      const uint32_t pos = find_key(*dicts[t], key);
      ids.push_back(pos == kNoPos ? SLG_NO_TERM : dicts[t]->map[pos]);
    }
    dist.push_back(d);
  };
  std::unordered_set<std::string> seen;
  const size_t fpl = rq.field_key.size();
  if (rq.kind == SLG_EXPAND_FUZZY) {
    emit(rq.exact_key, 0);
    if (!rq.scan) return;
    seen.insert(rq.exact_key);
    const std::string_view term = std::string_view(rq.exact_key).substr(fpl);
    size_t expansions = 0;
    for (uint32_t s = 0; s < n_segs; s++) {
      uint32_t lo, hi;
      prefix_range(*dicts[s], rq.range_key, lo, hi);
      for (uint32_t p = lo; p < hi; p++) {
        if (expansions >= rq.max_expansions) return;
        const std::string_view key = dicts[s]->key(p);
        if (key.size() <= fpl) continue;
        const std::string_view cand = key.substr(fpl);
        if (cand == term) continue;
        std::vector<uint32_t> cc;
        utf8_decode(cand.data(), cand.size(), &cc);
        const size_t cl = cc.size(), tl = rq.cps.size();
        if ((cl > tl ? cl - tl : tl - cl) > rq.max_edits) continue;
        size_t d;
        if (!ref_bounded_levenshtein(rq.cps, cc, rq.max_edits, &d) || d == 0) continue;
        if (seen.insert(std::string(key)).second) {
          emit(std::string(key), (uint8_t)d);
          expansions++;
        }
      }
    }
    return;
  }
  if (!rq.scan) return;
  for (uint32_t s = 0; s < n_segs; s++) {
    uint32_t lo, hi, expanded = 0;
    prefix_range(*dicts[s], rq.range_key, lo, hi);
    for (uint32_t p = lo; p < hi && expanded < rq.max_expansions; p++) {
      const std::string_view key = dicts[s]->key(p);
      if (key.size() <= fpl) continue;
      if (rq.kind == SLG_EXPAND_WILDCARD &&
          !slg::glob_match(rq.cps.data(), (uint32_t)rq.cps.size(), reinterpret_cast<const unsigned char *>(key.data()) + fpl,
                           (uint32_t)(key.size() - fpl)))
        continue;
      if (rq.kind == SLG_EXPAND_REGEX &&  // (the host build of the device's walk: this loop serves the timing tool only)
          !slg::regex_walk(rq.dfa.class_of, rq.dfa.table.data(), rq.dfa.accept.data(), rq.dfa.n_classes,
                           reinterpret_cast<const unsigned char *>(key.data()) + fpl, (uint32_t)(key.size() - fpl)))
        continue;
      if (!seen.insert(std::string(key)).second) continue;
      emit(std::string(key), 0);
      expanded++;
    }
  }
}
}  // namespace

extern "C" {

// -> an opaque sorted dictionary or NULL (err / code filled)
void *slgx_dict_build(uint32_t n_terms, const char *key_bytes, const uint32_t *key_offsets, char *err, uint32_t err_len,
                      int *code) {
  auto *d = new slgexpand::Dict();
  const int rc = guarded(err, err_len, [&] { slgexpand::build_dict(n_terms, key_bytes, key_offsets, *d); });
  if (code) *code = rc;
  if (rc != SLG_OK) {
    delete d;
    return nullptr;
  }
  return d;
}
void slgx_dict_free(void *d) { delete static_cast<slgexpand::Dict *>(d); }
// the sorted position -> term id map and the char counts ([n] each, either may be NULL) -> n
uint32_t slgx_dict_tables(const void *dict, uint32_t *map, uint8_t *nchars) {
  const auto &d = *static_cast<const slgexpand::Dict *>(dict);
  if (map) std::memcpy(map, d.map.data(), d.map.size() * 4);
  if (nchars) std::memcpy(nchars, d.nchars.data(), d.nchars.size());
  return d.n();
}
void slgx_prefix_range(const void *dict, const char *prefix, uint32_t len, uint32_t *lo, uint32_t *hi) {
  slgexpand::prefix_range(*static_cast<const slgexpand::Dict *>(dict), std::string_view(prefix ? prefix : "", len), *lo, *hi);
}
// the checks of a request; on success whether it scans, its clamped max_edits and its range key (range_cap bytes)
int slgx_check_request(const slg_expand_req *r, uint32_t *scan, uint32_t *max_edits, char *range_key, uint32_t range_cap,
                       uint32_t *range_len, char *err, uint32_t err_len) {
  return guarded(err, err_len, [&] {
    const slgexpand::Request q = slgexpand::check_request(*r, 0);
    *scan = q.scan;
    *max_edits = q.max_edits;
    *range_len = (uint32_t)q.range_key.size();
    std::memcpy(range_key, q.range_key.data(), std::min<size_t>(range_cap, q.range_key.size()));
  });
}
uint32_t slgx_rows_needed(const slg_expand_req *r, uint32_t seg) {
  try {
    return (uint32_t)slgexpand::rows_needed(slgexpand::check_request(*r, 0), seg);
  } catch (const slgplan::SlgError &) {
    return 0;
  }
}
// merge_request over hand-made device rows: segment s's rows are row_offsets[s] .. row_offsets[s + 1] - 1 of
// row_pos / row_dist.  out_ids [cap x n_segs], out_dist [cap]; *n_keys = the keys (also when cap is too small)
int slgx_merge(const slg_expand_req *r, const void *const *dicts, uint32_t n_segs, const uint32_t *row_offsets,
               const uint32_t *row_pos, const uint8_t *row_dist, uint32_t cap, uint32_t *out_ids, uint8_t *out_dist,
               uint32_t *n_keys, char *err, uint32_t err_len) {
  return guarded(err, err_len, [&] {
    const slgexpand::Request q = slgexpand::check_request(*r, 0);
    std::vector<slgexpand::Rows> rows(n_segs);
    for (uint32_t s = 0; s < n_segs; s++)
      rows[s] = slgexpand::Rows{row_pos + row_offsets[s], row_dist + row_offsets[s], row_offsets[s + 1] - row_offsets[s]};
    std::vector<uint32_t> ids;
    std::vector<uint8_t> dist;
    slgexpand::merge_request(q, reinterpret_cast<const slgexpand::Dict *const *>(dicts), n_segs, rows.data(), ids, dist);
    *n_keys = (uint32_t)dist.size();
    if (dist.size() > cap) throw slgplan::SlgError(SLG_ERR_INVALID, "slgx_merge: cap too small");
    if (!ids.empty()) std::memcpy(out_ids, ids.data(), ids.size() * 4);
    if (!dist.empty()) std::memcpy(out_dist, dist.data(), dist.size());
  });
}

// the scan's predicates, compiled for the host.  The distance of the kernel's banded form between the term's code
// points and a UTF-8 candidate (char counts within 2 of each other): <= max_edits, or slg::kExpandNoDistance
uint32_t slgx_banded_distance(const uint32_t *term, uint32_t n, const char *cand, uint32_t bytes, uint32_t max_edits) {
  const unsigned char *c = reinterpret_cast<const unsigned char *>(cand);
  return slg::banded_distance(term, (int)n, c, (int)slg::utf8_count(c, bytes), max_edits);
}
int slgx_glob_match(const uint32_t *pat, uint32_t n, const char *text, uint32_t bytes) {
  return slg::glob_match(pat, n, reinterpret_cast<const unsigned char *>(text), bytes) ? 1 : 0;
}

// The regex compiler (slg_regex.cpp) on a pattern of `len` bytes -> SLG_OK with the DFA (class_of [256], table
// [table_cap] filled if n_states x n_classes fits, accept [32]; any may be NULL), or the compiler's code with err
int slgx_regex_compile(const char *pattern, uint32_t len, uint32_t *n_states, uint32_t *n_classes, uint8_t *class_of,
                       uint8_t *table, uint32_t table_cap, uint8_t *accept, char *err, uint32_t err_len) {
  return guarded(err, err_len, [&] {
    std::vector<uint32_t> cps;
    if (!slgexpand::utf8_decode(pattern ? pattern : "", len, &cps)) throw slgplan::SlgError(SLG_ERR_INVALID, "regex: the pattern is not valid UTF-8");
    const slgregex::Dfa d = slgregex::compile(cps);
    if (n_states) *n_states = d.n_states;
    if (n_classes) *n_classes = d.n_classes;
    if (class_of) std::memcpy(class_of, d.class_of, 256);
    if (table && d.table.size() <= table_cap) std::memcpy(table, d.table.data(), d.table.size());
    if (accept) std::memcpy(accept, d.accept.data(), d.accept.size());
  });
}
// the device's walk (slg_expand_regex.hpp) compiled for the host, over one term -> 1 / 0
int slgx_regex_match(const uint8_t *class_of, const uint8_t *table, const uint8_t *accept, uint32_t n_classes,
                     const char *text, uint32_t bytes) {
  return slg::regex_walk(class_of, table, accept, n_classes, reinterpret_cast<const unsigned char *>(text), bytes) ? 1 : 0;
}
// regex_literal_prefix -> its bytes into out (cap bytes), *out_len its length; -1: the pattern is not valid UTF-8
int slgx_regex_literal_prefix(const char *pattern, uint32_t len, char *out, uint32_t cap, uint32_t *out_len) {
  std::vector<uint32_t> cps;
  if (!slgexpand::utf8_decode(pattern ? pattern : "", len, &cps)) return -1;
  std::string s;
  for (const uint32_t cp : slgregex::literal_prefix(cps)) slgregex::utf8_append(s, cp);
  *out_len = (uint32_t)s.size();
  std::memcpy(out, s.data(), std::min<size_t>(cap, s.size()));
  return 0;
}

// The reference's loop on the host for n_reqs requests over n_threads threads (requests dealt round robin).
// out_offsets [n_reqs + 1]; out_ids [cap x n_segs] / out_dist [cap] may be NULL (timing: the keys are counted only)
int slgx_reference_expand(const void *const *dicts, uint32_t n_segs, const slg_expand_req *reqs, uint32_t n_reqs,
                          uint32_t n_threads, uint32_t *out_offsets, uint32_t cap, uint32_t *out_ids, uint8_t *out_dist,
                          char *err, uint32_t err_len) {
  return guarded(err, err_len, [&] {
    std::vector<slgexpand::Request> rq;
    for (uint32_t i = 0; i < n_reqs; i++) rq.push_back(slgexpand::check_request(reqs[i], i));
    std::vector<std::vector<uint32_t>> ids(n_reqs);
    std::vector<std::vector<uint8_t>> dist(n_reqs);
    const auto *dd = reinterpret_cast<const slgexpand::Dict *const *>(dicts);
    const auto work = [&](uint32_t t) {
      for (uint32_t i = t; i < n_reqs; i += n_threads) ref_expand_one(rq[i], dd, n_segs, ids[i], dist[i]);
    };
    n_threads = std::max(1u, n_threads);
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < n_threads; t++) pool.emplace_back(work, t);
    work(0);
    for (auto &th : pool) th.join();
    uint32_t at = 0;
    for (uint32_t i = 0; i < n_reqs; i++) {
      out_offsets[i] = at;
      if (out_ids && out_dist && at + dist[i].size() <= cap && !dist[i].empty()) {
        std::memcpy(out_ids + (size_t)at * n_segs, ids[i].data(), ids[i].size() * 4);
        std::memcpy(out_dist + at, dist[i].data(), dist[i].size());
      }
      at += (uint32_t)dist[i].size();
    }
    out_offsets[n_reqs] = at;
    if (out_ids && at > cap) throw slgplan::SlgError(SLG_ERR_INVALID, "slgx_reference_expand: cap too small");
  });
}

}  // extern "C"
