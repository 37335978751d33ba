// slg_highlight.hip — slg_highlight_batch and slg_batch_highlight: the arguments checked and the field specs packed
// on the host (slg_highlight_host.cpp: one validation for both), then one staging path (highlight_run): the tables
// onto the device, the count pass and the scan, the totals back, the emit pass, the strings straight into the
// caller's arrays.  The two entry points differ only in where the hit rows come from.
#include "slg_host.hpp"

#include <chrono>

#include "slg_highlight.hpp"
#include "slg_highlight_host.hpp"

using namespace slghost;

namespace {
struct PhaseMs {
  double count = 0.0, emit = 0.0;
};
PhaseMs &phase_ms() {
  thread_local PhaseMs p;
  return p;
}
double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// what a state offers the validation
struct StateFacts {
  std::vector<uint32_t> seg_docs;
  std::vector<int32_t> fields;
  slghl::Against against() const {
    return slghl::Against{(uint32_t)seg_docs.size(), seg_docs.data(), fields.data(), (uint32_t)fields.size()};
  }
};
StateFacts facts_of(const IndexState &S) {
  StateFacts f;
  for (const auto &sh : S.segs) f.seg_docs.push_back(sh->n_docs);
  for (const auto &tf : S.text_fields) f.fields.push_back(tf.first);
  return f;
}

// the hit rows of a call: query q's are rows q_hit[q] .. q_hit[q] + q_rows[q] - 1 of seg / doc; host arrays
// (on_device false: uploaded here) or a batch's own (count: its device counts)
struct HitRows {
  std::vector<uint32_t> q_hit, q_rows;
  const uint32_t *seg, *doc;
  size_t n;
  bool on_device;
  const uint32_t *d_count;
};

// The staging path of both entry points.  pk: the validated specs; st: the stream the kernels are queued on (a
// batch's: behind its own kernels)
void highlight_run(const IndexState &S, BufPool *pool, hipStream_t st, slghl::Packed &pk, const HitRows &hr, slg_hl_out *out) {
  const uint32_t nq = (uint32_t)pk.q_spec.size() - 1u;
  for (size_t s = 0; s < pk.specs.size(); s++) {
    const TextFieldHost &tf = *S.text_fields.find(pk.field[s])->second;
    pk.specs[s].segs = tf.d_tsegs.as<const slg::TextSegDev>();
    pk.specs[s].n_segs = (uint32_t)S.segs.size();
  }
  const slghl::Slots sl = slghl::plan_slots(pk, hr.q_rows.data());
  const uint32_t n_slots = sl.n_slots, n_blocks = (uint32_t)sl.blocks.size();
  out->n_items = out->n_frags = 0u;
  out->text_bytes = 0u;
  phase_ms() = PhaseMs();
  if (n_slots == 0u) {
    if (!pk.size_query) out->offsets[0] = out->text_offsets[0] = 0u;
    return;
  }
  const auto t_count = std::chrono::steady_clock::now();
  Staging sg(pool, st);
  slg::HlParams p{};
  p.specs = sg.up(pk.specs.data(), pk.specs.size());
  p.blob = sg.up(pk.blob.data(), pk.blob.size());
  p.blocks = sg.up(sl.blocks.data(), sl.blocks.size());
  p.q_spec = sg.up(pk.q_spec.data(), pk.q_spec.size());
  p.q_slot = sg.up(sl.q_slot.data(), sl.q_slot.size());
  p.q_hit = sg.up(hr.q_hit.data(), hr.q_hit.size());
  p.q_rows = sg.up(hr.q_rows.data(), hr.q_rows.size());
  p.hit_seg = hr.on_device ? hr.seg : sg.up(hr.seg, hr.n);
  p.hit_doc = hr.on_device ? hr.doc : sg.up(hr.doc, hr.n);
  p.count = hr.d_count;
  p.status = sg.up<uint8_t>(nullptr, n_slots);
  p.n_frags = sg.up<uint32_t>(nullptr, n_slots);
  p.item_bytes = sg.up<uint32_t>(nullptr, n_slots);
  p.frag_start = sg.up<uint32_t>(nullptr, (size_t)n_slots * slg::kHlMaxFragments);
  p.frag_len = sg.up<uint32_t>(nullptr, (size_t)n_slots * slg::kHlMaxFragments);
  p.n_slots = n_slots;
  p.slot_frag0 = sg.up<uint32_t>(nullptr, (size_t)n_slots + 1u);
  p.slot_text0 = sg.up<uint64_t>(nullptr, (size_t)n_slots + 1u);
  hipLaunchKernelGGL(slg::hl_count_kernel, dim3(n_blocks), dim3(slg::kHlThreads), 0, st, p);
  SLG_HIP(hipGetLastError());
  hipLaunchKernelGGL(slg::hl_scan_kernel, dim3(1), dim3(slg::kHlScanThreads), 0, st, p);
  SLG_HIP(hipGetLastError());
  uint32_t total_frags = 0u;
  uint64_t total_text = 0u;
  std::vector<uint32_t> count(hr.d_count ? nq : 0u);
  sg.down(&total_frags, p.slot_frag0 + n_slots, 1);
  sg.down(&total_text, p.slot_text0 + n_slots, 1);
  sg.down(count.data(), hr.d_count, count.size());
  SLG_HIP(hipStreamSynchronize(st));
  phase_ms().count = ms_since(t_count);

  // the items: every slot, or (a batch's rows) the slots of the rows in front of count[q]
  uint64_t n_items = 0;
  for (uint32_t q = 0; q < nq; q++)
    n_items += (uint64_t)(hr.d_count ? std::min(count[q], hr.q_rows[q]) : hr.q_rows[q]) * (pk.q_spec[q + 1] - pk.q_spec[q]);
  if (total_text >= (1ull << 32)) throw SlgError(SLG_ERR_UNSUPPORTED, "highlight: 2^32 or more bytes of output in one call");
  out->n_items = (uint32_t)n_items;
  out->n_frags = total_frags;
  out->text_bytes = total_text;
  if (pk.size_query) return;
  SLG_REQUIRE(n_items <= out->item_capacity, "highlight: item_capacity " + std::to_string(out->item_capacity) + " is too small");
  SLG_REQUIRE(total_frags <= out->frag_capacity, "highlight: frag_capacity " + std::to_string(out->frag_capacity) + " is too small");
  SLG_REQUIRE(total_text <= out->text_capacity, "highlight: text_capacity " + std::to_string(out->text_capacity) + " is too small");

  const auto t_emit = std::chrono::steady_clock::now();
  p.frag_cap = total_frags;
  p.text_cap = total_text;
  p.out_text_offsets = sg.up<uint32_t>(nullptr, total_frags);
  p.out_text = sg.up<uint8_t>(nullptr, total_text);
  if (total_frags) {
    hipLaunchKernelGGL(slg::hl_emit_kernel, dim3(n_blocks), dim3(slg::kHlThreads), 0, st, p);
    SLG_HIP(hipGetLastError());
  }
  std::vector<uint8_t> status(n_slots);
  std::vector<uint32_t> n_frags(n_slots);
  sg.down(status.data(), p.status, n_slots);
  sg.down(n_frags.data(), p.n_frags, n_slots);
  sg.down(out->text_offsets, p.out_text_offsets, total_frags);
  sg.down(reinterpret_cast<uint8_t *>(out->text), p.out_text, total_text);
  SLG_HIP(hipStreamSynchronize(st));
  out->text_offsets[total_frags] = (uint32_t)total_text;
  uint32_t item = 0u, frag = 0u;
  for (uint32_t slot = 0; slot < n_slots; slot++) {
    if (status[slot] == slg::kHlNoRow) continue;  // (such a slot has no fragments)
    if (item >= n_items) throw SlgError(SLG_ERR_INTERNAL, "highlight: the count pass marked more rows than the batch counts");
    out->status[item] = status[slot];
    out->offsets[item++] = frag;
    frag += n_frags[slot];
  }
  if (item != n_items || frag != total_frags) throw SlgError(SLG_ERR_INTERNAL, "highlight: the passes disagree about the items");
  out->offsets[item] = frag;
  phase_ms().emit = ms_since(t_emit);
}
}  // namespace

extern "C" {

int slg_highlight_batch(slg_index *ix, uint32_t n_queries, const uint32_t *hit_offsets, const uint32_t *hit_seg,
                        const uint32_t *hit_doc, const uint32_t *spec_offsets, const slg_hl_spec *specs, slg_hl_out *out) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    const auto S = ix->snapshot();
    const StateFacts facts = facts_of(*S);
    const slghl::HostHits hits{hit_offsets, hit_seg, hit_doc};
    slghl::Packed pk = slghl::validate(n_queries, spec_offsets, specs, &hits, facts.against(), out);
    HitRows hr{{}, {}, hit_seg, hit_doc, hit_offsets[n_queries], false, nullptr};
    for (uint32_t q = 0; q < n_queries; q++) {
      hr.q_hit.push_back(hit_offsets[q]);
      hr.q_rows.push_back(hit_offsets[q + 1] - hit_offsets[q]);
    }
    DeviceGuard g(ix->device);
    hipStream_t st;
    {
      std::lock_guard<std::mutex> lk(ix->mu);
      st = ix->stream;
    }
    highlight_run(*S, &ix->pool, st, pk, hr, out);
  });
}

int slg_batch_highlight(slg_batch *b, const uint32_t *spec_offsets, const slg_hl_spec *specs, slg_hl_out *out) {
  return guarded([&] {
    SLG_REQUIRE_LIVE(b);
    SLG_REQUIRE(b->launched && b->d_out_doc && b->d_out_seg && b->d_out_count, "highlight: the batch has not run");
    const IndexState &S = *b->snap;
    const StateFacts facts = facts_of(S);
    slghl::Packed pk = slghl::validate(b->nq, spec_offsets, specs, nullptr, facts.against(), out);
    HitRows hr{{}, {}, b->d_out_seg, b->d_out_doc, (size_t)b->nq * b->k, true, b->d_out_count};
    for (uint32_t q = 0; q < b->nq; q++) {
      hr.q_hit.push_back(q * b->k);
      hr.q_rows.push_back(b->k);
    }
    DeviceGuard g(b->idx->device);
    highlight_run(S, &b->idx->pool, locked_stream(b), pk, hr, out);
  });
}

int slg_highlight_phase_ms(slg_index *ix, double *count_ms, double *emit_ms) {
  return guarded([&] {
    SLG_REQUIRE(ix != nullptr, "index is NULL");
    if (count_ms) *count_ms = phase_ms().count;
    if (emit_ms) *emit_ms = phase_ms().emit;
  });
}

}  // extern "C"
