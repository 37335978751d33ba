// slg_suggest_host.hpp — the host side of slg_suggest_batch (slg_suggest_host.cpp): pure host code, linked into
// libsearchlite_gpu.so and, behind a small test C ABI (slg_suggest_capi.cpp), into lib/libslg_plan.so.  It checks
// a request, derives its cap and the prefix whose range is scanned, and clips a plain request's range to the keys
// the reference can visit.  It computes no score, no distance and compares no texts.
#pragma once

#include "slg_expand_merge.hpp"
#include "slg_suggest.hpp"

namespace slgsuggest {

using slgexpand::SlgError;

struct Request {
  std::string field_key;      // "field:"
  std::string range_key;      // "field:" + the prefix whose range is scanned
  std::vector<uint32_t> cps;  // code points of the term
  uint32_t field_chars = 0;   // chars of field_key
  uint32_t size = 0, cap = 0, max_edits = 0;
  bool fuzzy = false;
  bool scan = false;          // false: no options whatever the dictionaries hold
};
// Throws SLG_ERR_INVALID (struct_size, NULL strings, invalid UTF-8) or SLG_ERR_UNSUPPORTED (more than
// SLG_MAX_EXPAND_CHARS chars; a fuzzy request of size above SLG_MAX_SUGGEST_CANDIDATES)
Request check_request(const slg_suggest_req &r, uint32_t index);

slg::SuggestReqDev device_request(const Request &rq);

// A plain request visits keys until `cap` of them have passed.  nonzero[p] = the keys in front of sorted position
// p with df != 0; only the bare key "field:", the range's first, can have df != 0 and not pass.  -> the end of the
// shortest prefix of [lo, hi) that holds cap + 1 keys with df != 0, or hi
uint32_t clip_plain(const std::vector<uint32_t> &nonzero, uint32_t lo, uint32_t hi, uint32_t cap);

}  // namespace slgsuggest
