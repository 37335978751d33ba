// slg_highlight_host.hpp — the host side of slg_highlight_batch / slg_batch_highlight (slg_highlight_host.cpp):
// pure host code, linked into libsearchlite_gpu.so and, behind a small test C ABI (slg_highlight_capi.cpp), into
// lib/libslg_plan.so.  It checks a call's arguments (validate: the one validation of both entry points), packs the
// field specs into the tables the kernels read, lays a call's workgroups and item slots out (plan_slots), and holds
// the sequential highlighter (highlight_text): hl_match_at of slg_highlight.hpp one byte at a time, what a caller
// without the device runs and what tools/highlight_time.py times against.
#pragma once

#include <string>
#include <vector>

#include "../../include/searchlite_gpu.h"
#include "slg_plan.hpp"  // SlgError
#define SLG_HL_NO_KERNELS
#include "slg_highlight.hpp"

namespace slghl {

using slgplan::SlgError;

// the host hits of slg_highlight_batch (a batch's rows are on the device: nothing to check)
struct HostHits {
  const uint32_t *offsets, *seg, *doc;
};
// what the specs and hits are checked against: the segments' doc counts and the registered text field ids
struct Against {
  uint32_t n_segs;
  const uint32_t *seg_docs;
  const int32_t *fields;
  uint32_t n_fields;
};
struct Packed {
  std::vector<slg::HlSpecDev> specs;  // segs / n_segs not set: the caller binds `field` to its state
  std::vector<int32_t> field;         // [specs.size()] text field id
  std::vector<uint8_t> blob;
  std::vector<uint32_t> q_spec;       // [nq + 1]
  bool size_query = false;
};
// Throws SLG_ERR_INVALID or SLG_ERR_UNSUPPORTED as searchlite_gpu.h lists them; hits null: the batch form
Packed validate(uint32_t nq, const uint32_t *spec_offsets, const slg_hl_spec *specs, const HostHits *hits, const Against &ag,
                const slg_hl_out *out);

// the call's geometry: query q has rows[q] hit rows; its item slots are q_slot[q] + row * n_specs(q) + spec, its
// workgroups one per (spec, kHlWaves rows)
struct Slots {
  std::vector<uint32_t> q_slot;  // [nq]
  std::vector<slg::HlBlockDev> blocks;
  uint32_t n_slots = 0;
};
Slots plan_slots(const Packed &pk, const uint32_t *rows);

// the table of spec s unpacked as the kernels hold it in LDS
void unpack_table(const Packed &pk, uint32_t s, slg::HlTable &t);
// highlight_fragments on one ASCII text, sequentially
void highlight_text(const Packed &pk, uint32_t s, const slg::HlTable &t, const uint8_t *text, uint32_t len,
                    std::vector<std::string> &out);

}  // namespace slghl
