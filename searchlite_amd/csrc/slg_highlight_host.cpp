// slg_highlight_host.cpp — see slg_highlight_host.hpp.  Pure host code: no HIP header, builds with g++.
#include "slg_highlight_host.hpp"

#include <algorithm>
#include <cstring>

namespace slghl {

static_assert(slg::kHlMaxTerms == SLG_MAX_HL_TERMS && slg::kHlMaxPhrases == SLG_MAX_HL_PHRASES &&
                  slg::kHlMaxPhraseWords == SLG_MAX_PHRASE_TERMS && slg::kHlMaxWordBytes == SLG_MAX_EXPAND_CHARS &&
                  slg::kHlMaxTag == SLG_MAX_HL_TAG && slg::kHlMaxFragment == SLG_MAX_HL_FRAGMENT &&
                  slg::kHlMaxFragments == SLG_MAX_HL_FRAGMENTS && slg::kHlOk == SLG_HL_OK && slg::kHlHost == SLG_HL_HOST &&
                  slg::kHlNoText == SLG_HL_NO_TEXT,
              "the highlighter's constants as the ABI states them");

namespace {
[[noreturn]] void invalid(const std::string &m) { throw SlgError(SLG_ERR_INVALID, "highlight: " + m); }
[[noreturn]] void unsupported(const std::string &m) { throw SlgError(SLG_ERR_UNSUPPORTED, "highlight: " + m); }

void check_out(const slg_hl_out *out, bool &size_query) {
  if (!out) invalid("out is NULL");
  if (out->struct_size != sizeof(slg_hl_out)) invalid("out: struct_size is not sizeof(slg_hl_out)");
  const int given = (out->status != nullptr) + (out->offsets != nullptr) + (out->text_offsets != nullptr) + (out->text != nullptr);
  if (given != 0 && given != 4) invalid("out: status, offsets, text_offsets and text are all NULL (a size query) or all given");
  size_query = given == 0;
}

// one spec onto the end of pk; at: "query Q field spec F: "
void pack_spec(const slg_hl_spec &sp, const std::string &at, const Against &ag, Packed &pk) {
  if (sp.struct_size != sizeof(slg_hl_spec)) invalid(at + "struct_size is not sizeof(slg_hl_spec)");
  if (std::find(ag.fields, ag.fields + ag.n_fields, sp.text_field) == ag.fields + ag.n_fields)
    invalid(at + "unknown text field id " + std::to_string(sp.text_field));
  if (sp.n_phrases && !sp.phrase_offsets) invalid(at + "phrase_offsets is NULL");
  if (sp.n_phrases && sp.phrase_offsets[0] != 0u) invalid(at + "phrase_offsets does not start at 0");
  for (uint32_t p = 0; p < sp.n_phrases; p++) {
    if (sp.phrase_offsets[p + 1] < sp.phrase_offsets[p]) invalid(at + "phrase_offsets decrease");
    if (sp.phrase_offsets[p + 1] == sp.phrase_offsets[p]) invalid(at + "phrase " + std::to_string(p) + " has no words");
  }
  const uint64_t n_pw = sp.n_phrases ? sp.phrase_offsets[sp.n_phrases] : 0u, n_words = (uint64_t)sp.n_terms + n_pw;
  if (n_words && !sp.word_offsets) invalid(at + "word_offsets is NULL");
  if (n_words && sp.word_offsets[0] != 0u) invalid(at + "word_offsets does not start at 0");
  for (uint64_t w = 0; w < n_words; w++) {
    if (sp.word_offsets[w + 1] < sp.word_offsets[w]) invalid(at + "word_offsets decrease");
    if (sp.word_offsets[w + 1] == sp.word_offsets[w])
      invalid(at + (w < sp.n_terms ? "term " + std::to_string(w) + " is empty" : "a phrase holds an empty word"));
  }
  if (n_words && !sp.word_bytes) invalid(at + "word_bytes is NULL");
  if (sp.pre_len && !sp.pre_tag) invalid(at + "pre_tag is NULL");
  if (sp.post_len && !sp.post_tag) invalid(at + "post_tag is NULL");
  // the limits: the CPU path
  if (sp.n_terms > SLG_MAX_HL_TERMS) unsupported(at + std::to_string(sp.n_terms) + " terms (more than SLG_MAX_HL_TERMS)");
  if (sp.n_phrases > SLG_MAX_HL_PHRASES) unsupported(at + std::to_string(sp.n_phrases) + " phrases (more than SLG_MAX_HL_PHRASES)");
  for (uint32_t p = 0; p < sp.n_phrases; p++)
    if (sp.phrase_offsets[p + 1] - sp.phrase_offsets[p] > SLG_MAX_PHRASE_TERMS)
      unsupported(at + "phrase " + std::to_string(p) + " has more than SLG_MAX_PHRASE_TERMS words");
  for (uint64_t w = 0; w < n_words; w++) {
    const uint32_t a = sp.word_offsets[w], e = sp.word_offsets[w + 1];
    if (e - a > SLG_MAX_EXPAND_CHARS) unsupported(at + "a word of " + std::to_string(e - a) + " bytes (more than SLG_MAX_EXPAND_CHARS)");
    for (uint32_t i = a; i < e; i++)
      if (!slg::hl_is_word((uint8_t)sp.word_bytes[i]))
        unsupported(at + "a word holds a byte outside [0-9A-Za-z_] (the reference's \\b and case folding then depend on Unicode tables)");
  }
  if (sp.pre_len > SLG_MAX_HL_TAG || sp.post_len > SLG_MAX_HL_TAG) unsupported(at + "a tag of more than SLG_MAX_HL_TAG bytes");
  if (sp.fragment_size > SLG_MAX_HL_FRAGMENT)
    unsupported(at + "fragment_size " + std::to_string(sp.fragment_size) + " (more than SLG_MAX_HL_FRAGMENT)");
  if (sp.number_of_fragments > SLG_MAX_HL_FRAGMENTS)
    unsupported(at + "number_of_fragments " + std::to_string(sp.number_of_fragments) + " (more than SLG_MAX_HL_FRAGMENTS)");

  slg::HlSpecDev d{};
  d.n_terms = sp.n_terms;
  d.n_phrases = sp.n_phrases;
  d.n_words = (uint32_t)n_words;
  d.fs = sp.fragment_size;
  d.nf = sp.number_of_fragments;
  d.pre_len = sp.pre_len;
  d.post_len = sp.post_len;
  pk.blob.resize((pk.blob.size() + 3u) & ~(size_t)3u);
  d.blob = (uint32_t)pk.blob.size();
  // the phrases' words first, then the terms: the order hl_match_at tries them in
  std::vector<uint16_t> word_off(n_words + 1u, 0u);
  std::vector<uint8_t> phrase_first(sp.n_phrases + 1u, 0u), bytes;
  auto push_word = [&](uint64_t w, uint32_t slot, bool first) {
    const uint32_t a = sp.word_offsets[w], e = sp.word_offsets[w + 1];
    for (uint32_t i = a; i < e; i++) bytes.push_back(slg::hl_fold((uint8_t)sp.word_bytes[i]));
    word_off[slot + 1] = (uint16_t)bytes.size();
    if (first) d.len_mask[(e - a) >> 5] |= 1u << ((e - a) & 31u);
  };
  uint32_t slot = 0;
  for (uint32_t p = 0; p < sp.n_phrases; p++) {
    phrase_first[p] = (uint8_t)slot;
    for (uint32_t w = sp.phrase_offsets[p]; w < sp.phrase_offsets[p + 1]; w++, slot++) push_word(sp.n_terms + w, slot, w == sp.phrase_offsets[p]);
  }
  phrase_first[sp.n_phrases] = (uint8_t)slot;
  for (uint32_t w = 0; w < sp.n_terms; w++, slot++) push_word(w, slot, true);
  d.word_bytes = (uint32_t)bytes.size();
  const auto append = [&](const void *p, size_t n) {
    if (n) pk.blob.insert(pk.blob.end(), static_cast<const uint8_t *>(p), static_cast<const uint8_t *>(p) + n);
  };
  append(word_off.data(), word_off.size() * 2u);
  append(phrase_first.data(), phrase_first.size());
  append(bytes.data(), bytes.size());
  append(sp.pre_tag, sp.pre_len);
  append(sp.post_tag, sp.post_len);
  if (pk.blob.size() >= (1ull << 31)) unsupported("the batch's word tables are too large for one call");
  pk.specs.push_back(d);
  pk.field.push_back(sp.text_field);
}
}  // namespace

Packed validate(uint32_t nq, const uint32_t *spec_offsets, const slg_hl_spec *specs, const HostHits *hits, const Against &ag,
                const slg_hl_out *out) {
  Packed pk;
  check_out(out, pk.size_query);
  if (!spec_offsets) invalid("spec_offsets is NULL");
  if (spec_offsets[0] != 0u) invalid("spec_offsets does not start at 0");
  for (uint32_t q = 0; q < nq; q++)
    if (spec_offsets[q + 1] < spec_offsets[q]) invalid("spec_offsets decrease");
  if (spec_offsets[nq] && !specs) invalid("specs is NULL");
  if (hits) {
    if (!hits->offsets) invalid("hit_offsets is NULL");
    if (hits->offsets[0] != 0u) invalid("hit_offsets does not start at 0");
    for (uint32_t q = 0; q < nq; q++)
      if (hits->offsets[q + 1] < hits->offsets[q]) invalid("hit_offsets decrease");
    if (hits->offsets[nq] && (!hits->seg || !hits->doc)) invalid("hit_seg or hit_doc is NULL");
    for (uint32_t q = 0; q < nq; q++)
      for (uint32_t h = hits->offsets[q]; h < hits->offsets[q + 1]; h++) {
        if (hits->seg[h] >= ag.n_segs) invalid("query " + std::to_string(q) + ": a hit's segment " + std::to_string(hits->seg[h]) + " is out of range");
        if (hits->doc[h] >= ag.seg_docs[hits->seg[h]])
          invalid("query " + std::to_string(q) + ": a hit's doc " + std::to_string(hits->doc[h]) + " is out of range");
      }
  }
  pk.q_spec.assign(spec_offsets, spec_offsets + nq + 1u);
  for (uint32_t q = 0; q < nq; q++)
    for (uint32_t s = spec_offsets[q]; s < spec_offsets[q + 1]; s++)
      pack_spec(specs[s], "query " + std::to_string(q) + " field spec " + std::to_string(s - spec_offsets[q]) + ": ", ag, pk);
  return pk;
}

Slots plan_slots(const Packed &pk, const uint32_t *rows) {
  Slots sl;
  const uint32_t nq = (uint32_t)pk.q_spec.size() - 1u;
  sl.q_slot.resize(nq);
  uint64_t slots = 0;
  for (uint32_t q = 0; q < nq; q++) {
    sl.q_slot[q] = (uint32_t)slots;
    const uint32_t n_specs = pk.q_spec[q + 1] - pk.q_spec[q];
    slots += (uint64_t)rows[q] * n_specs;
    if (slots >= (1ull << 28) || sl.blocks.size() >= (1u << 28)) unsupported("too many items for one call");
    for (uint32_t s = pk.q_spec[q]; s < pk.q_spec[q + 1]; s++)
      for (uint32_t r = 0; r < rows[q]; r += slg::kHlWaves) sl.blocks.push_back(slg::HlBlockDev{q, s, r});
  }
  sl.n_slots = (uint32_t)slots;
  return sl;
}

void unpack_table(const Packed &pk, uint32_t s, slg::HlTable &t) {
  const slg::HlSpecDev &d = pk.specs[s];
  const uint8_t *src = pk.blob.data() + d.blob;
  std::memcpy(t.len_mask, d.len_mask, sizeof(t.len_mask));
  std::memcpy(t.word_off, src, 2u * (d.n_words + 1u));
  std::memcpy(t.phrase_first, src + 2u * (d.n_words + 1u), d.n_phrases + 1u);
  if (d.word_bytes) std::memcpy(t.bytes, src + 2u * (d.n_words + 1u) + d.n_phrases + 1u, d.word_bytes);
}

void highlight_text(const Packed &pk, uint32_t s, const slg::HlTable &t, const uint8_t *text, uint32_t len,
                    std::vector<std::string> &out) {
  const slg::HlSpecDev &d = pk.specs[s];
  if (!len || !d.n_words) return;
  const char *pre = reinterpret_cast<const char *>(pk.blob.data()) + d.blob + 2u * (d.n_words + 1u) + d.n_phrases + 1u + d.word_bytes;
  const char *post = pre + d.pre_len;
  const char *tx = reinterpret_cast<const char *>(text);
  uint32_t offset = 0;
  for (uint32_t n = 0; n < d.nf; n++) {
    uint32_t me = 0;
    const uint32_t ms = slg::hl_next_match(t, d.n_phrases, d.n_words, text, 0u, len, offset, me);
    if (ms == slg::kHlNone) break;
    const uint32_t start = slg::hl_fragment_start(ms, d.fs), end = slg::hl_fragment_end(start, d.fs, len);
    std::string frag;
    uint32_t pos = start, fe = 0;
    for (;;) {
      const uint32_t fsm = slg::hl_next_match(t, d.n_phrases, d.n_words, text, start, end, pos, fe);
      if (fsm == slg::kHlNone) break;
      frag.append(tx + pos, fsm - pos).append(pre, d.pre_len).append(tx + fsm, fe - fsm).append(post, d.post_len);
      pos = fe;
    }
    frag.append(tx + pos, end - pos);
    out.push_back(std::move(frag));
    offset = me;
  }
}

}  // namespace slghl
