// slg_suggest_host.cpp — see slg_suggest_host.hpp.  Pure host code: no HIP header, builds with g++.
#include "slg_suggest_host.hpp"

#include <algorithm>

namespace slgsuggest {

Request check_request(const slg_suggest_req &r, uint32_t index) {
  const std::string at = "suggest: request " + std::to_string(index) + ": ";
  if (r.struct_size != sizeof(slg_suggest_req)) throw SlgError(SLG_ERR_INVALID, at + "struct_size is not sizeof(slg_suggest_req)");
  if (!r.field && r.field_len) throw SlgError(SLG_ERR_INVALID, at + "field is NULL");
  if (!r.term && r.term_len) throw SlgError(SLG_ERR_INVALID, at + "term is NULL");
  Request q;
  std::vector<uint32_t> field_cps;
  if (!slgexpand::utf8_decode(r.field, r.field_len, &field_cps)) throw SlgError(SLG_ERR_INVALID, at + "field is not valid UTF-8");
  if (!slgexpand::utf8_decode(r.term, r.term_len, &q.cps)) throw SlgError(SLG_ERR_INVALID, at + "term is not valid UTF-8");
  if (q.cps.size() > SLG_MAX_EXPAND_CHARS)
    throw SlgError(SLG_ERR_UNSUPPORTED, at + "a term of " + std::to_string(q.cps.size()) + " chars (more than SLG_MAX_EXPAND_CHARS)");
  q.fuzzy = r.has_fuzzy != 0;
  if (q.fuzzy && r.size > SLG_MAX_SUGGEST_CANDIDATES)
    throw SlgError(SLG_ERR_UNSUPPORTED, at + "a fuzzy request of size " + std::to_string(r.size) + " (its cap is above SLG_MAX_SUGGEST_CANDIDATES)");
  q.field_key.assign(r.field ? r.field : "", r.field_len);
  q.field_key.push_back(':');
  q.field_chars = (uint32_t)field_cps.size() + 1;
  q.size = r.size;
  const std::string_view term(r.term ? r.term : "", r.term_len);
  size_t prefix_bytes = term.size();
  if (q.fuzzy) {
    q.max_edits = std::min<uint32_t>(r.max_edits, 2u);                                                    // :1832
    q.scan = r.size > 0 && q.cps.size() >= r.min_length && r.max_expansions > 0 && q.max_edits > 0;       // :1948, :1829, :1833
    q.cap = slg::suggest_fuzzy_cap(r.max_expansions, r.size);                                             // :1840-1841
    const size_t chars = std::min<size_t>(r.prefix_length, q.cps.size());                                 // :1836-1837
    prefix_bytes = 0;
    for (size_t c = 0; c < chars; c++) {
      prefix_bytes++;
      while (prefix_bytes < term.size() && (static_cast<unsigned char>(term[prefix_bytes]) & 0xC0u) == 0x80u) prefix_bytes++;
    }
  } else {
    q.scan = r.size > 0;                     // :1948
    q.cap = slg::suggest_plain_cap(r.size);  // :1793-1795
  }
  q.range_key = q.field_key;
  q.range_key.append(term.substr(0, prefix_bytes));
  return q;
}

slg::SuggestReqDev device_request(const Request &rq) {
  slg::SuggestReqDev d{};
  d.fuzzy = rq.fuzzy ? 1u : 0u;
  d.max_edits = rq.max_edits;
  d.n_chars = (uint32_t)rq.cps.size();
  d.field_bytes = (uint32_t)rq.field_key.size();
  d.field_chars = rq.field_chars;
  d.skip_bytes = (uint32_t)(rq.range_key.size() - rq.field_key.size());
  d.cap = rq.cap;
  d.size = rq.size;
  std::copy(rq.cps.begin(), rq.cps.end(), d.cp);
  return d;
}

uint32_t clip_plain(const std::vector<uint32_t> &nonzero, uint32_t lo, uint32_t hi, uint32_t cap) {
  const uint64_t want = (uint64_t)nonzero[lo] + cap + 1u;
  const auto it = std::lower_bound(nonzero.begin() + lo, nonzero.begin() + hi + 1, want,
                                   [](uint32_t have, uint64_t w) { return have < w; });
  return (uint32_t)std::min<size_t>((size_t)(it - nonzero.begin()), hi);
}

}  // namespace slgsuggest
