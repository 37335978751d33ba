// highlight_sanitize.cpp — a stand-alone program (its own main) that drives the highlighter's host translation unit
// (csrc/slg_highlight_host.cpp through the test C ABI of csrc/slg_highlight_capi.cpp) with valid and malformed spec
// arrays: the validation, the packing of the word tables and the sequential highlighter.  tests/test_highlight_ref.py
// builds it with -fsanitize=address,undefined and runs it on the host; every array here is a heap allocation of
// exactly its stated size, so a read one element past any of them is reported.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/searchlite_gpu.h"

extern "C" {
int slgx_hl_validate(uint32_t nq, int batch_form, const uint32_t *hit_offsets, const uint32_t *hit_seg, const uint32_t *hit_doc,
                     const uint32_t *spec_offsets, const slg_hl_spec *specs, uint32_t n_segs, const uint32_t *seg_docs,
                     const int32_t *fields, uint32_t n_fields, const slg_hl_out *out, uint32_t *n_specs, uint32_t *blob_bytes,
                     char *err, uint32_t err_len);
int slgx_hl_reference(uint32_t n_items, const uint64_t *text_offsets, const uint8_t *text_bytes, const uint32_t *item_spec,
                      uint32_t n_specs, const slg_hl_spec *specs, uint32_t n_threads, slg_hl_out *out, char *err, uint32_t err_len);
}

namespace {
int failures = 0;
void expect(bool ok, const char *what) {
  if (!ok) {
    std::printf("FAILED: %s\n", what);
    failures++;
  }
}

// a spec whose arrays live on the heap, each exactly as long as the spec says
struct Spec {
  std::vector<std::string> terms;
  std::vector<std::vector<std::string>> phrases;
  std::string pre = "<em>", post = "</em>";
  uint32_t fs = 160, nf = 1;
  int32_t field = 0;
  std::unique_ptr<uint32_t[]> word_offsets, phrase_offsets;
  std::unique_ptr<char[]> bytes, pre_b, post_b;
  Spec() = default;
  Spec(const Spec &o) : terms(o.terms), phrases(o.phrases), pre(o.pre), post(o.post), fs(o.fs), nf(o.nf), field(o.field) {}
  Spec &operator=(const Spec &o) {
    terms = o.terms, phrases = o.phrases, pre = o.pre, post = o.post, fs = o.fs, nf = o.nf, field = o.field;
    return *this;
  }
  slg_hl_spec make() {
    std::vector<std::string> words = terms;
    std::vector<uint32_t> po{0u};
    for (const auto &p : phrases) {
      words.insert(words.end(), p.begin(), p.end());
      po.push_back(po.back() + (uint32_t)p.size());
    }
    std::string blob;
    word_offsets.reset(new uint32_t[words.size() + 1]);
    word_offsets[0] = 0u;
    for (size_t w = 0; w < words.size(); w++) {
      blob += words[w];
      word_offsets[w + 1] = (uint32_t)blob.size();
    }
    phrase_offsets.reset(new uint32_t[po.size()]);
    std::memcpy(phrase_offsets.get(), po.data(), po.size() * 4);
    bytes.reset(new char[blob.size()]);
    std::memcpy(bytes.get(), blob.data(), blob.size());
    pre_b.reset(new char[pre.size()]);
    std::memcpy(pre_b.get(), pre.data(), pre.size());
    post_b.reset(new char[post.size()]);
    std::memcpy(post_b.get(), post.data(), post.size());
    slg_hl_spec s{};
    s.struct_size = sizeof(slg_hl_spec);
    s.text_field = field;
    s.n_terms = (uint32_t)terms.size();
    s.n_phrases = (uint32_t)phrases.size();
    s.phrase_offsets = phrase_offsets.get();
    s.word_offsets = word_offsets.get();
    s.word_bytes = bytes.get();
    s.pre_tag = pre_b.get();
    s.post_tag = post_b.get();
    s.pre_len = (uint32_t)pre.size();
    s.post_len = (uint32_t)post.size();
    s.fragment_size = fs;
    s.number_of_fragments = nf;
    return s;
  }
};

int validate_one(const slg_hl_spec &s, std::string *msg = nullptr) {
  std::unique_ptr<uint32_t[]> so(new uint32_t[2]{0u, 1u}), ho(new uint32_t[2]{0u, 1u}), hs(new uint32_t[1]{0u}), hd(new uint32_t[1]{2u}),
      docs(new uint32_t[1]{3u});
  std::unique_ptr<int32_t[]> fields(new int32_t[1]{0});
  std::unique_ptr<slg_hl_spec[]> specs(new slg_hl_spec[1]{s});
  slg_hl_out out{};
  out.struct_size = sizeof(slg_hl_out);
  char err[256] = {0};
  const int rc = slgx_hl_validate(1u, 0, ho.get(), hs.get(), hd.get(), so.get(), specs.get(), 1u, docs.get(), fields.get(), 1u, &out,
                                  nullptr, nullptr, err, sizeof(err));
  if (msg) *msg = err;
  return rc;
}

// the texts under the specs (item i: text i, spec i % n_specs) through the sequential highlighter, size query first
std::vector<std::string> reference(const std::vector<std::string> &texts, std::vector<Spec> &sp, std::vector<uint8_t> *status = nullptr) {
  const uint32_t n = (uint32_t)texts.size(), ns = (uint32_t)sp.size();
  std::unique_ptr<uint64_t[]> offs(new uint64_t[n + 1]);
  std::string blob;
  offs[0] = 0;
  for (uint32_t i = 0; i < n; i++) {
    blob += texts[i];
    offs[i + 1] = blob.size();
  }
  std::unique_ptr<uint8_t[]> bytes(new uint8_t[blob.size()]);
  std::memcpy(bytes.get(), blob.data(), blob.size());
  std::unique_ptr<uint32_t[]> item_spec(new uint32_t[n]);
  for (uint32_t i = 0; i < n; i++) item_spec[i] = i % ns;
  std::unique_ptr<slg_hl_spec[]> specs(new slg_hl_spec[ns]);
  for (uint32_t s = 0; s < ns; s++) specs[s] = sp[s].make();
  slg_hl_out out{};
  out.struct_size = sizeof(slg_hl_out);
  char err[256] = {0};
  int rc = slgx_hl_reference(n, offs.get(), bytes.get(), item_spec.get(), ns, specs.get(), 3u, &out, err, sizeof(err));
  expect(rc == SLG_OK, err);
  if (rc != SLG_OK) return {};
  std::unique_ptr<uint8_t[]> st(new uint8_t[out.n_items]);
  std::unique_ptr<uint32_t[]> io(new uint32_t[out.n_items + 1]), to(new uint32_t[out.n_frags + 1]);
  std::unique_ptr<char[]> text(new char[out.text_bytes]);
  out.item_capacity = out.n_items;
  out.frag_capacity = out.n_frags;
  out.text_capacity = out.text_bytes;
  out.status = st.get();
  out.offsets = io.get();
  out.text_offsets = to.get();
  out.text = text.get();
  rc = slgx_hl_reference(n, offs.get(), bytes.get(), item_spec.get(), ns, specs.get(), 2u, &out, err, sizeof(err));
  expect(rc == SLG_OK, err);
  std::vector<std::string> frags;
  for (uint32_t f = 0; rc == SLG_OK && f < out.n_frags; f++) frags.emplace_back(text.get() + to[f], to[f + 1] - to[f]);
  if (status) status->assign(st.get(), st.get() + out.n_items);
  // capacities one too small are refused, nothing is written past them
  if (rc == SLG_OK && out.text_bytes) {
    out.text_capacity = out.text_bytes - 1;
    expect(slgx_hl_reference(n, offs.get(), bytes.get(), item_spec.get(), ns, specs.get(), 1u, &out, err, sizeof(err)) == SLG_ERR_INVALID,
           "a text capacity one too small is refused");
  }
  return frags;
}
}  // namespace

int main() {
  // ---- valid specs: the results by hand -----------------------------------------------------------------------
  {
    std::vector<Spec> sp(1);
    sp[0].terms = {"systems"};
    sp[0].pre = sp[0].post = "**";
    sp[0].fs = 120;
    const auto f = reference({"Rust is a systems programming language", ""}, sp);
    expect(f.size() == 1 && f[0] == "Rust is a **systems** programming language", "the reference's own test");
  }
  {
    std::vector<Spec> sp(2);
    sp[0].terms = {"new"};
    sp[0].phrases = {{"new", "york"}};
    sp[0].nf = 8;
    sp[0].fs = 12;
    sp[1].terms = {"go", "ust"};
    sp[1].fs = 8;
    sp[1].pre = "";
    std::vector<uint8_t> status;
    const auto f = reference({"New   York, new yorker", "xxxxrust go", "caf\xC3\xA9 new", "", "x"}, sp, &status);
    expect(status.size() == 5 && status[2] == SLG_HL_HOST && status[0] == SLG_HL_OK && status[3] == SLG_HL_OK, "statuses");
    expect(f.size() == 3 && f[0] == "<em>New   York</em>, " && f[1] == "York, <em>new</em> yo" && f[2] == "ust</em> go</em>",
           "phrase, fall-through and the cut word");
  }
  {  // the table at its limits, a text that ends inside every kind of look-ahead
    std::vector<Spec> sp(1);
    for (uint32_t t = 0; t < SLG_MAX_HL_TERMS - 1; t++) sp[0].terms.push_back("t" + std::to_string(t));
    sp[0].terms.push_back(std::string(SLG_MAX_EXPAND_CHARS, 'L'));
    for (uint32_t p = 0; p < SLG_MAX_HL_PHRASES; p++) {
      sp[0].phrases.emplace_back();
      for (uint32_t w = 0; w < SLG_MAX_PHRASE_TERMS; w++) sp[0].phrases.back().push_back("p" + std::to_string(p) + "w" + std::to_string(w));
    }
    sp[0].pre = std::string(SLG_MAX_HL_TAG, '[');
    sp[0].post = "";
    sp[0].fs = SLG_MAX_HL_FRAGMENT;
    sp[0].nf = SLG_MAX_HL_FRAGMENTS;
    std::string full;
    for (const auto &w : sp[0].phrases[7]) full += w + " ";
    const std::string longw(SLG_MAX_EXPAND_CHARS, 'l');
    const auto f = reference({full, full.substr(0, full.size() - 4), "p7w0", "p7w0 ", longw, longw + "l", "t30 " + longw + " t5"}, sp);
    expect(f.size() == 5, "limits: the full phrase, the long word, and the terms around it");
  }
  // ---- malformed specs: every refusal, and no read outside the arrays ------------------------------------------
  {
    Spec ok;
    ok.terms = {"rust"};
    ok.phrases = {{"new", "york"}};
    slg_hl_spec s = ok.make();
    std::string msg;
    expect(validate_one(s) == SLG_OK, "a valid spec");
    s.struct_size = 8;
    expect(validate_one(s) == SLG_ERR_INVALID, "struct_size");
    s = ok.make();
    s.text_field = 9;
    expect(validate_one(s) == SLG_ERR_INVALID, "unknown field");
    s = ok.make();
    s.word_offsets = nullptr;
    expect(validate_one(s) == SLG_ERR_INVALID, "NULL word_offsets");
    s = ok.make();
    s.phrase_offsets = nullptr;
    expect(validate_one(s) == SLG_ERR_INVALID, "NULL phrase_offsets");
    s = ok.make();
    s.word_bytes = nullptr;
    expect(validate_one(s) == SLG_ERR_INVALID, "NULL word_bytes");
    s = ok.make();
    s.pre_tag = nullptr;
    expect(validate_one(s) == SLG_ERR_INVALID, "NULL pre_tag");
    s = ok.make();
    const_cast<uint32_t *>(s.word_offsets)[2] = 1u;
    expect(validate_one(s) == SLG_ERR_INVALID, "decreasing word_offsets");
    s = ok.make();
    const_cast<uint32_t *>(s.phrase_offsets)[1] = 0u;
    expect(validate_one(s) == SLG_ERR_INVALID, "a phrase without words");
    Spec empty_word = ok;
    empty_word.phrases = {{"new", "", "york"}};
    expect(validate_one(empty_word.make(), &msg) == SLG_ERR_INVALID && msg.find("empty word") != std::string::npos, "an empty word in a phrase");
    Spec empty_term = ok;
    empty_term.terms = {"rust", ""};
    expect(validate_one(empty_term.make()) == SLG_ERR_INVALID, "an empty term");
    Spec bad = ok;
    bad.terms = {"caf\xC3\xA9"};
    expect(validate_one(bad.make(), &msg) == SLG_ERR_UNSUPPORTED && msg.find("query 0 field spec 0") != std::string::npos, "a non-word byte");
    bad = ok;
    bad.terms = {"new york"};
    expect(validate_one(bad.make()) == SLG_ERR_UNSUPPORTED, "a space in a word");
    bad = ok;
    bad.terms.assign(SLG_MAX_HL_TERMS + 1, "a");
    expect(validate_one(bad.make()) == SLG_ERR_UNSUPPORTED, "too many terms");
    bad = ok;
    bad.phrases.assign(SLG_MAX_HL_PHRASES + 1, {"a"});
    expect(validate_one(bad.make()) == SLG_ERR_UNSUPPORTED, "too many phrases");
    bad = ok;
    bad.phrases = {std::vector<std::string>(SLG_MAX_PHRASE_TERMS + 1, "a")};
    expect(validate_one(bad.make()) == SLG_ERR_UNSUPPORTED, "too many words in a phrase");
    bad = ok;
    bad.terms = {std::string(SLG_MAX_EXPAND_CHARS + 1, 'a')};
    expect(validate_one(bad.make()) == SLG_ERR_UNSUPPORTED, "a word too long");
    bad = ok;
    bad.post = std::string(SLG_MAX_HL_TAG + 1, 'x');
    expect(validate_one(bad.make()) == SLG_ERR_UNSUPPORTED, "a tag too long");
    bad = ok;
    bad.fs = SLG_MAX_HL_FRAGMENT + 1;
    expect(validate_one(bad.make()) == SLG_ERR_UNSUPPORTED, "fragment_size");
    bad = ok;
    bad.nf = SLG_MAX_HL_FRAGMENTS + 1;
    expect(validate_one(bad.make()) == SLG_ERR_UNSUPPORTED, "number_of_fragments");
  }
  if (failures) return 1;
  std::printf("highlight_sanitize ok\n");
  return 0;
}
