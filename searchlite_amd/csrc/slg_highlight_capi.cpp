// slg_highlight_capi.cpp — a small C ABI over the highlighter's host side (slg_highlight_host.cpp) for the CPU unit
// tests (tests/test_highlight_ref.py, tests/test_highlight_args.py) and tools/highlight_time.py: the validation of
// both entry points against hand-made index facts, and the sequential highlighter over texts given directly (what a
// caller without the device runs).  Built into lib/libslg_plan.so with g++; NOT part of libsearchlite_gpu.so's
// exported surface.
#include <cstring>
#include <memory>
#include <thread>

#include "slg_highlight_host.hpp"

namespace {
template <typename F>
int guarded(char *err, uint32_t err_len, F &&f) {
  try {
    f();
    return SLG_OK;
  } catch (const slghl::SlgError &e) {
    if (err && err_len) {
      std::strncpy(err, e.what(), err_len - 1);
      err[err_len - 1] = 0;
    }
    return e.code;
  }
}
}  // namespace

extern "C" {

// slghl::validate as the entry points call it: hit_offsets NULL with batch_form != 0 (a batch's rows), the index
// facts given by hand.  On success *n_specs and *blob_bytes say what was packed
int slgx_hl_validate(uint32_t nq, int batch_form, const uint32_t *hit_offsets, const uint32_t *hit_seg, const uint32_t *hit_doc,
                     const uint32_t *spec_offsets, const slg_hl_spec *specs, uint32_t n_segs, const uint32_t *seg_docs,
                     const int32_t *fields, uint32_t n_fields, const slg_hl_out *out, uint32_t *n_specs, uint32_t *blob_bytes,
                     char *err, uint32_t err_len) {
  return guarded(err, err_len, [&] {
    const slghl::HostHits hits{hit_offsets, hit_seg, hit_doc};
    const slghl::Packed pk = slghl::validate(nq, spec_offsets, specs, batch_form ? nullptr : &hits,
                                             slghl::Against{n_segs, seg_docs, fields, n_fields}, out);
    if (n_specs) *n_specs = (uint32_t)pk.specs.size();
    if (blob_bytes) *blob_bytes = (uint32_t)pk.blob.size();
  });
}

// The sequential highlighter: item i is the text text_bytes[text_offsets[i] .. text_offsets[i + 1]) under spec
// item_spec[i] of `specs` (text_field is not looked at), the items dealt round robin over n_threads threads.  out as
// slg_highlight_batch fills it (a size query too); a text with a byte >= 0x80 is SLG_HL_HOST
int slgx_hl_reference(uint32_t n_items, const uint64_t *text_offsets, const uint8_t *text_bytes, const uint32_t *item_spec,
                      uint32_t n_specs, const slg_hl_spec *specs, uint32_t n_threads, slg_hl_out *out, char *err, uint32_t err_len) {
  return guarded(err, err_len, [&] {
    std::vector<int32_t> fields(n_specs);
    for (uint32_t s = 0; s < n_specs; s++) fields[s] = specs[s].text_field;
    const uint32_t one_query[2] = {0u, n_specs};
    const slghl::Packed pk = slghl::validate(1u, one_query, specs, nullptr, slghl::Against{0u, nullptr, fields.data(), n_specs}, out);
    std::vector<std::unique_ptr<slg::HlTable>> tables(n_specs);
    for (uint32_t s = 0; s < n_specs; s++) {
      tables[s] = std::make_unique<slg::HlTable>();
      slghl::unpack_table(pk, s, *tables[s]);
    }
    for (uint32_t i = 0; i < n_items; i++)
      if (item_spec[i] >= n_specs || text_offsets[i + 1] < text_offsets[i] || text_offsets[i + 1] - text_offsets[i] >= (1ull << 31))
        throw slghl::SlgError(SLG_ERR_INVALID, "slgx_hl_reference: item " + std::to_string(i) + " is malformed");
    std::vector<std::vector<std::string>> frags(n_items);
    std::vector<uint8_t> status(n_items, (uint8_t)SLG_HL_OK);
    const auto work = [&](uint32_t t) {
      for (uint32_t i = t; i < n_items; i += n_threads) {
        const uint8_t *tx = text_bytes + text_offsets[i];
        const uint32_t len = (uint32_t)(text_offsets[i + 1] - text_offsets[i]);
        bool ascii = true;
        for (uint32_t b = 0; b < len && ascii; b++) ascii = tx[b] < 0x80u;
        if (!ascii) {
          status[i] = (uint8_t)SLG_HL_HOST;
          continue;
        }
        slghl::highlight_text(pk, item_spec[i], *tables[item_spec[i]], tx, len, frags[i]);
      }
    };
    n_threads = std::max(1u, n_threads);
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < n_threads; t++) pool.emplace_back(work, t);
    work(0);
    for (auto &th : pool) th.join();
    uint64_t n_frags = 0, bytes = 0;
    for (uint32_t i = 0; i < n_items; i++)
      for (const std::string &f : frags[i]) {
        n_frags++;
        bytes += f.size();
      }
    out->n_items = n_items;
    out->n_frags = (uint32_t)n_frags;
    out->text_bytes = bytes;
    if (pk.size_query) return;
    if (n_items > out->item_capacity || n_frags > out->frag_capacity || bytes > out->text_capacity)
      throw slghl::SlgError(SLG_ERR_INVALID, "slgx_hl_reference: a capacity is too small");
    uint32_t f = 0;
    uint64_t at = 0;
    for (uint32_t i = 0; i < n_items; i++) {
      out->status[i] = status[i];
      out->offsets[i] = f;
      for (const std::string &s : frags[i]) {
        out->text_offsets[f++] = (uint32_t)at;
        std::memcpy(out->text + at, s.data(), s.size());
        at += s.size();
      }
    }
    out->offsets[n_items] = f;
    out->text_offsets[f] = (uint32_t)at;
  });
}

}  // extern "C"
