// slg_expand_merge.cpp — see slg_expand_merge.hpp.  Pure host code: no HIP header, builds with g++.
#include "slg_expand_merge.hpp"

#include <algorithm>
#include <numeric>
#include <unordered_set>

namespace slgexpand {

bool utf8_decode(const char *s, size_t len, std::vector<uint32_t> *cps) {
  const unsigned char *p = reinterpret_cast<const unsigned char *>(s);
  size_t i = 0;
  while (i < len) {
    const uint32_t b0 = p[i];
    uint32_t cp, extra, min;
    if (b0 < 0x80u) {
      cp = b0, extra = 0, min = 0;
    } else if (b0 >= 0xC2u && b0 < 0xE0u) {
      cp = b0 & 0x1Fu, extra = 1, min = 0x80u;
    } else if (b0 >= 0xE0u && b0 < 0xF0u) {
      cp = b0 & 0x0Fu, extra = 2, min = 0x800u;
    } else if (b0 >= 0xF0u && b0 < 0xF5u) {
      cp = b0 & 0x07u, extra = 3, min = 0x10000u;
    } else {
      return false;
    }
    if (i + extra >= len + (extra == 0)) return false;  // (extra continuation bytes must exist)
    for (uint32_t k = 1; k <= extra; k++) {
      if ((p[i + k] & 0xC0u) != 0x80u) return false;
      cp = (cp << 6) | (p[i + k] & 0x3Fu);
    }
    if (cp < min || cp > 0x10FFFFu || (cp >= 0xD800u && cp < 0xE000u)) return false;
    if (cps) cps->push_back(cp);
    i += extra + 1;
  }
  return true;
}

void build_dict(uint32_t n_terms, const char *key_bytes, const uint32_t *key_offsets, Dict &out) {
  if (!key_offsets) throw SlgError(SLG_ERR_INVALID, "set_terms: key_offsets is NULL");
  for (uint32_t i = 0; i < n_terms; i++)
    if (key_offsets[i + 1] < key_offsets[i]) throw SlgError(SLG_ERR_INVALID, "set_terms: key_offsets decrease at key " + std::to_string(i));
  if (!key_bytes && n_terms && key_offsets[n_terms] > key_offsets[0]) throw SlgError(SLG_ERR_INVALID, "set_terms: key_bytes is NULL");
  std::vector<std::string_view> keys(n_terms);
  for (uint32_t i = 0; i < n_terms; i++) {
    keys[i] = std::string_view(key_bytes + key_offsets[i], key_offsets[i + 1] - key_offsets[i]);
    if (keys[i].find(':') == std::string_view::npos)
      throw SlgError(SLG_ERR_INVALID, "set_terms: key " + std::to_string(i) + " has no ':' (keys are \"field:term\")");
    if (!utf8_decode(keys[i].data(), keys[i].size(), nullptr))
      throw SlgError(SLG_ERR_INVALID, "set_terms: key " + std::to_string(i) + " is not valid UTF-8");
  }
  std::vector<uint32_t> order(n_terms);
  std::iota(order.begin(), order.end(), 0u);
  const auto less = [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; };  // (char_traits<char>: bytes as unsigned)
  if (!std::is_sorted(order.begin(), order.end(), less)) std::sort(order.begin(), order.end(), less);
  for (uint32_t i = 1; i < n_terms; i++)
    if (keys[order[i - 1]] == keys[order[i]])
      throw SlgError(SLG_ERR_INVALID, "set_terms: keys " + std::to_string(order[i - 1]) + " and " + std::to_string(order[i]) + " are equal");
  out = Dict();
  out.offs.assign(1, 0u);
  out.offs.reserve((size_t)n_terms + 1);
  out.nchars.reserve(n_terms);
  for (uint32_t i = 0; i < n_terms; i++) {
    const std::string_view k = keys[order[i]];
    out.bytes.append(k);
    out.offs.push_back((uint32_t)out.bytes.size());
    size_t chars = 0;
    for (const char ch : k) chars += (static_cast<unsigned char>(ch) & 0xC0u) != 0x80u;
    out.nchars.push_back((uint8_t)std::min<size_t>(chars, 255));
  }
  out.map = std::move(order);
}

void prefix_range(const Dict &d, std::string_view prefix, uint32_t &lo, uint32_t &hi) {
  // keys below the range compare less than prefix; keys of the range start with it; both are prefixes of the
  // sorted order, so two partition points
  uint32_t a = 0, b = d.n();
  while (a < b) {
    const uint32_t mid = a + (b - a) / 2;
    if (d.key(mid) < prefix) a = mid + 1; else b = mid;
  }
  lo = a;
  b = d.n();
  while (a < b) {
    const uint32_t mid = a + (b - a) / 2;
    if (d.key(mid).substr(0, prefix.size()) == prefix) a = mid + 1; else b = mid;
  }
  hi = a;
}

uint32_t find_key(const Dict &d, std::string_view key) {
  uint32_t a = 0, b = d.n();
  while (a < b) {
    const uint32_t mid = a + (b - a) / 2;
    if (d.key(mid) < key) a = mid + 1; else b = mid;
  }
  return a < d.n() && d.key(a) == key ? a : kNoPos;
}

Request check_request(const slg_expand_req &r, uint32_t index) {
  const std::string at = "expand: request " + std::to_string(index) + ": ";
  if (r.struct_size != sizeof(slg_expand_req)) throw SlgError(SLG_ERR_INVALID, at + "struct_size is not sizeof(slg_expand_req)");
  if (r.kind != SLG_EXPAND_FUZZY && r.kind != SLG_EXPAND_PREFIX && r.kind != SLG_EXPAND_WILDCARD && r.kind != SLG_EXPAND_REGEX)
    throw SlgError(SLG_ERR_INVALID, at + "unknown kind " + std::to_string(r.kind));
  if (!r.field && r.field_len) throw SlgError(SLG_ERR_INVALID, at + "field is NULL");
  if (!r.term && r.term_len) throw SlgError(SLG_ERR_INVALID, at + "term is NULL");
  Request q;
  q.kind = r.kind;
  std::vector<uint32_t> field_cps;
  if (!utf8_decode(r.field, r.field_len, &field_cps)) throw SlgError(SLG_ERR_INVALID, at + "field is not valid UTF-8");
  if (!utf8_decode(r.term, r.term_len, &q.cps)) throw SlgError(SLG_ERR_INVALID, at + "term is not valid UTF-8");
  if (q.cps.size() > SLG_MAX_EXPAND_CHARS)
    throw SlgError(SLG_ERR_UNSUPPORTED, at + "a term or pattern of " + std::to_string(q.cps.size()) + " chars (more than SLG_MAX_EXPAND_CHARS)");
  if (r.max_expansions > SLG_MAX_EXPANSIONS)
    throw SlgError(SLG_ERR_UNSUPPORTED, at + "max_expansions " + std::to_string(r.max_expansions) + " is above SLG_MAX_EXPANSIONS");
  q.field_key.assign(r.field ? r.field : "", r.field_len);
  q.field_key.push_back(':');
  q.field_chars = (uint32_t)field_cps.size() + 1;
  std::string_view term(r.term ? r.term : "", r.term_len);
  q.exact_key = q.field_key;
  q.exact_key.append(term);
  q.max_expansions = r.max_expansions;
  size_t prefix_bytes = term.size();
  if (r.kind == SLG_EXPAND_FUZZY) {
    q.max_edits = std::min<uint32_t>(r.max_edits, 2u);                               // :1415
    q.scan = q.cps.size() >= r.min_length && r.max_expansions > 0 && q.max_edits > 0;  // :1412, :1140-1143
    const size_t chars = std::min<size_t>(r.prefix_length, q.cps.size());            // :1416-1417, char_prefix
    prefix_bytes = 0;
    for (size_t c = 0; c < chars; c++) {
      prefix_bytes++;
      while (prefix_bytes < term.size() && (static_cast<unsigned char>(term[prefix_bytes]) & 0xC0u) == 0x80u) prefix_bytes++;
    }
  } else {
    q.scan = r.max_expansions > 0;  // :1173, :1241, :1331
    if (r.kind == SLG_EXPAND_WILDCARD) prefix_bytes = std::min(term.find_first_of("*?"), term.size());  // :1212-1214
  }
  std::string regex_prefix;
  if (r.kind == SLG_EXPAND_REGEX) {
    try {
      q.dfa = slgregex::compile(q.cps);
    } catch (const SlgError &e) {
      throw SlgError(e.code, at + e.what());
    }
    for (const uint32_t cp : slgregex::literal_prefix(q.cps)) slgregex::utf8_append(regex_prefix, cp);  // :1285-1320
    term = regex_prefix;  // (not a prefix of the pattern's bytes: an escaped char stands as itself)
    prefix_bytes = term.size();
  }
  q.range_key = q.field_key;
  q.range_key.append(term.substr(0, prefix_bytes));
  return q;
}

void merge_request(const Request &rq, const Dict *const *dicts, uint32_t n_segs, const Rows *rows,
                   std::vector<uint32_t> &ids, std::vector<uint8_t> &dist) {
  // a key's row: its id in the segment it was found in from the map, in the others by a lookup of its bytes
  const auto emit = [&](std::string_view key, uint32_t found_seg, uint32_t found_pos, uint8_t d) {
    for (uint32_t t = 0; t < n_segs; t++) {
      const uint32_t pos = t == found_seg ? found_pos : find_key(*dicts[t], key);
      ids.push_back(pos == kNoPos ? SLG_NO_TERM : dicts[t]->map[pos]);
    }
    dist.push_back(d);
  };
  std::unordered_set<std::string_view> seen;  // (views into the dictionaries' host copies and the request)
  if (rq.kind == SLG_EXPAND_FUZZY) {
    emit(rq.exact_key, kNoPos, kNoPos, 0);  // :1403-1411
    if (!rq.scan) return;
    seen.insert(rq.exact_key);
    uint32_t expansions = 0;
    for (uint32_t s = 0; s < n_segs; s++)
      for (uint32_t i = 0; i < rows[s].n; i++) {
        if (expansions >= rq.max_expansions) return;  // :1428, :1458 the global cap
        const std::string_view key = dicts[s]->key(rows[s].pos[i]);
        if (!seen.insert(key).second) continue;
        emit(key, s, rows[s].pos[i], rows[s].dist[i]);
        expansions++;
      }
    return;
  }
  if (!rq.scan) return;
  for (uint32_t s = 0; s < n_segs; s++) {
    uint32_t expanded = 0;  // :1182, :1252 the cap of this segment
    for (uint32_t i = 0; i < rows[s].n && expanded < rq.max_expansions; i++) {
      const std::string_view key = dicts[s]->key(rows[s].pos[i]);
      if (!seen.insert(key).second) continue;
      emit(key, s, rows[s].pos[i], 0);
      expanded++;
    }
  }
}

}  // namespace slgexpand
