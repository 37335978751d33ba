// slg_expand_merge.hpp — the host side of slg_expand_batch (slg_expand_merge.cpp): pure host code, linked into
// libsearchlite_gpu.so and, behind a small test C ABI (slg_expand_capi.cpp), into lib/libslg_plan.so, so it is
// unit-tested and sanitized without a GPU.  It checks and sorts a segment's dictionary, checks a request and finds
// its range, and runs the reference's sequential loop (api/reader.rs:1164-1283, 1322-1373, 1394-1465) over the rows the
// device scan produced: the seen set by key bytes, the global or per-segment cap, then the row of term ids.  It
// never computes a distance and never scans a dictionary.
#pragma once

#include <cstdint>
#include <string>
#include <string_view>
#include <vector>

#include "../../include/searchlite_gpu.h"
#include "slg_plan.hpp"  // SlgError
#include "slg_regex.hpp"

namespace slgexpand {

using slgplan::SlgError;

constexpr uint32_t kNoPos = 0xFFFFFFFFu;

// a segment's dictionary in byte order: the host copy (the device holds bytes, offs, map and nchars too)
struct Dict {
  std::string bytes;             // the sorted keys back to back
  std::vector<uint32_t> offs;    // [n + 1]
  std::vector<uint32_t> map;     // sorted position -> term id
  std::vector<uint8_t> nchars;   // chars of each key, saturating at 255
  uint32_t n() const { return (uint32_t)map.size(); }
  std::string_view key(uint32_t pos) const { return std::string_view(bytes).substr(offs[pos], offs[pos + 1] - offs[pos]); }
};

// the code points of valid UTF-8 (false: not valid — overlong forms, surrogates and values past U+10FFFF
// included, as Rust's str refuses them); cps may be null
bool utf8_decode(const char *s, size_t len, std::vector<uint32_t> *cps);

// slg_index_set_terms: check the keys and build the sorted dictionary.  Throws SLG_ERR_INVALID for NULL arrays,
// decreasing offsets, a key without ':', invalid UTF-8, duplicate keys
void build_dict(uint32_t n_terms, const char *key_bytes, const uint32_t *key_offsets, Dict &out);

// [lo, hi): the sorted positions of the keys that start with prefix
void prefix_range(const Dict &d, std::string_view prefix, uint32_t &lo, uint32_t &hi);
// the sorted position of key, or kNoPos
uint32_t find_key(const Dict &d, std::string_view key);

// a checked request
struct Request {
  int kind = 0;
  std::string field_key;       // "field:"
  std::string exact_key;       // "field:term" (fuzzy: key 0)
  std::string range_key;       // "field:" + the prefix whose range is scanned
  std::vector<uint32_t> cps;   // code points of the term / pattern
  uint32_t field_chars = 0;    // chars of field_key
  uint32_t max_expansions = 0, max_edits = 0;
  bool scan = false;           // false: nothing to scan (fuzzy: the exact key alone; else no keys)
  slgregex::Dfa dfa;           // regex: the compiled pattern (slg_regex.hpp)
};
// Throws SLG_ERR_INVALID (struct_size, kind, NULL strings, invalid UTF-8) or SLG_ERR_UNSUPPORTED (more than
// SLG_MAX_EXPAND_CHARS chars, max_expansions above SLG_MAX_EXPANSIONS), and for a regex request whatever
// slgregex::compile throws, whatever max_expansions is (the reference's planner compiles the pattern first,
// query/planner.rs:599); `index`: the request's, for the message
Request check_request(const slg_expand_req &r, uint32_t index);

// R: the passing keys of segment seg's range the reference can consume
inline uint64_t rows_needed(const Request &rq, uint32_t seg) {
  return rq.kind == SLG_EXPAND_FUZZY ? rq.max_expansions : (uint64_t)(seg + 1) * rq.max_expansions;
}

// the device's rows of one (request, segment): the first n passing keys of the range in dictionary order
struct Rows {
  const uint32_t *pos = nullptr;
  const uint8_t *dist = nullptr;
  uint32_t n = 0;
};

// The reference's loop over rows[0 .. n_segs) -> the request's keys in its order: per key a row of n_segs term
// ids appended to ids, and its distance to dist
void merge_request(const Request &rq, const Dict *const *dicts, uint32_t n_segs, const Rows *rows,
                   std::vector<uint32_t> &ids, std::vector<uint8_t> &dist);

}  // namespace slgexpand
