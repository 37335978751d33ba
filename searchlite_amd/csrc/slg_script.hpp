// slg_script.hpp — script_score at the root of the score tree (slg_batch_prepare_script): the reference's
// CompiledScript::evaluate (query/script.rs:69-146) and its ScriptScore node (api/reader.rs:577-612) as one kernel
// between the scoring kernel and the select.  The semantics in full: include/searchlite_gpu.h.  In short, per
// candidate:
//   the program runs in reverse Polish order on a stack of f64: PUSH_CONST a constant, PUSH_FIELD the doc's first
//   value of a column or 0.0 (script.rs:80-87), PUSH_SCORE the base score as f64; ADD / SUB / MUL pop b, pop a, push
//   a op b, NONE when the result is not finite (:89-115); DIV is NONE when b == 0.0 (-0.0 too) before it divides,
//   and when the quotient is not finite (:116-127); NEG negates (:128-135).  v = (float)top, NONE when not finite
//   (reader.rs:596); score = v * boost in f32, NONE when not finite (:599-602).  NONE drops the doc.
//   All f64 operations are single IEEE operations (the unit is built with -ffp-contract=off and without fast-math).
//
// Shape: fscore_kernel's (slg_fscore.hpp) — candidates mode, one wave per slice, four per workgroup, one candidate
// per lane, 64 per chunk, clause_candidate / clause_keep / clause_finish of slg_clause.hpp with the invariant of the
// in-place store stated there.  The query's record, its instructions with their constants and the column addresses
// of the slice's segment are wave-uniform and read through the constant address space (scalar loads), so op, slot
// and field are scalar branches.  Per candidate and DISTINCT field of the query the vector loads are offsets[doc]
// and offsets[doc + 1] (none when the column is stored without offsets) and values[first]: a field pushed several
// times is gathered once.
//
// The stack.  The positions of a reverse Polish program are static, so the planner records with every instruction
// the slot it works at (ScriptInstr::code) and the wave never tracks a stack pointer.  The slots and the eight field
// values are named registers, chosen by written-out compares against the uniform slot (script_pick): nothing goes to
// scratch (the resource usage of the build: profiles/script_resource_usage.txt).  The highest live slot is held in a
// register of its own, `top`: an operator then selects ONE operand (the other is the top) and stores nothing, and
// only a push puts a value away — about half the selects of a form that reads and writes every operand by slot.  A
// lane whose doc is NONE keeps executing the uniform program; the flag accumulates.
//
// One instantiation: the 8-slot kernel needs fewer than 64 VGPRs, the most a wave may hold at full occupancy, so a
// second one for shallow programs would gain no occupancy.
#pragma once

#include "slg_clause.hpp"
#include "slg_fscore.hpp"  // (fscore_base)

namespace slg {

constexpr int kScriptThreads = 256;  // four waves = four slices per workgroup

// the values of searchlite_gpu.h's enum (checked in slg_script.hip)
constexpr uint32_t kScPushConst = 0, kScPushField = 1, kScPushScore = 2, kScAdd = 3, kScSub = 4, kScMul = 5, kScDiv = 6,
                   kScNeg = 7;

struct ScriptParams {
  BoolFilterParams c;          // the slices, the candidates and q_scored (queries and terms: unused, null)
  const ScriptQuery *queries;  // [nq]
  const ScriptInstr *instrs;   // the instructions of all queries
  const ColumnDev *cols;       // [fields of the batch][n_segs]
};

// One of eight f64 registers, chosen by a wave-uniform slot.  The registers travel BY VALUE and the compares are
// written out: no address of a stack object ever exists, so nothing can be left in memory (an array under an
// unrolled loop, or a struct behind a reference, is still addressed at run time when the compiler promotes stack
// objects, and then stays in scratch or LDS).
__device__ __forceinline__ double script_pick(uint32_t at, double r0, double r1, double r2, double r3, double r4, double r5,
                                              double r6, double r7) {
  double v = r0;
  v = at == 1u ? r1 : v;
  v = at == 2u ? r2 : v;
  v = at == 3u ? r3 : v;
  v = at == 4u ? r4 : v;
  v = at == 5u ? r5 : v;
  v = at == 6u ? r6 : v;
  v = at == 7u ? r7 : v;
  return v;
}

// the doc's first value of the column of row `row` of the column table (wave-uniform), 0.0 without one; not loaded
// at all when the query has no such field (`used`, wave-uniform).  UNI: the segment is wave-uniform (fscore_u64)
template <bool UNI>
__device__ __forceinline__ double script_field(const ColumnDev *cols, uint32_t n_segs, uint32_t seg, uint32_t row, bool used,
                                               uint32_t doc, bool live) {
  typedef const __attribute__((address_space(1))) uint32_t *gu32_t;
  typedef const __attribute__((address_space(1))) double *gf64_t;
  double v = 0.0;
  if (used) {
    const ColumnDev col = load_const(cols + ((size_t)rfl(row) * n_segs + seg));
    const uint64_t offs = fscore_u64<UNI>((uint64_t)(uintptr_t)col.offs), vals = fscore_u64<UNI>((uint64_t)(uintptr_t)col.vals);
    uint32_t first = doc, end = doc + 1u;
    if (offs != 0ull && live) {  // (a live doc is below the segment's n_docs: offsets has n_docs + 1 entries)
      first = ((gu32_t)(uintptr_t)offs)[doc];
      end = ((gu32_t)(uintptr_t)offs)[doc + 1u];
    }
    if (live && first < end) v = ((gf64_t)(uintptr_t)vals)[first];
  }
  return v;
}

// One candidate through the program of its query: script * boost, and in `none` whether the script gives the doc no
// score (the doc is dropped).  prog: the query's instructions; n_instrs, n_fields: the query's, wave-uniform
template <bool UNI>
__device__ __forceinline__ float script_candidate(const ScriptQuery &sq, const ScriptInstr *const prog, const uint32_t n_instrs,
                                                  const uint32_t n_fields, const ColumnDev *const cols, const uint32_t n_segs,
                                                  const uint32_t seg, const uint32_t doc, const bool live,
                                                  const float base_f32, bool &none_out) {
  const double base_score = (double)base_f32;
  // the doc's first value of every distinct field of the query, 0.0 without one
  const double f0 = script_field<UNI>(cols, n_segs, seg, sq.col[0], n_fields > 0u, doc, live);
  const double f1 = script_field<UNI>(cols, n_segs, seg, sq.col[1], n_fields > 1u, doc, live);
  const double f2 = script_field<UNI>(cols, n_segs, seg, sq.col[2], n_fields > 2u, doc, live);
  const double f3 = script_field<UNI>(cols, n_segs, seg, sq.col[3], n_fields > 3u, doc, live);
  const double f4 = script_field<UNI>(cols, n_segs, seg, sq.col[4], n_fields > 4u, doc, live);
  const double f5 = script_field<UNI>(cols, n_segs, seg, sq.col[5], n_fields > 5u, doc, live);
  const double f6 = script_field<UNI>(cols, n_segs, seg, sq.col[6], n_fields > 6u, doc, live);
  const double f7 = script_field<UNI>(cols, n_segs, seg, sq.col[7], n_fields > 7u, doc, live);
  // The stack: `top` is its highest live slot, s0 .. s6 the slots below it (slot 7 can only ever be the top).  An
  // instruction's result is the new top: a push at slot `at` first puts the old top, slot at - 1, away; an operator
  // at slot `at` reads a = slot at from the registers and b = slot at + 1 = the top; NEG works on the top alone.
  double top = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0;
  bool none = false;
  for (uint32_t i = 0; i < n_instrs; i++) {
    const ScriptInstr in = load_const(prog + i);
    const uint32_t code = rfl(in.code);
    const uint32_t op = code & 0xFFu, at = (code >> 8) & 0xFFu;
    double r;
    if (op <= kScPushScore) {
      const uint32_t below = at - 1u;  // (at 0: no slot)
      s0 = below == 0u ? top : s0;
      s1 = below == 1u ? top : s1;
      s2 = below == 2u ? top : s2;
      s3 = below == 3u ? top : s3;
      s4 = below == 4u ? top : s4;
      s5 = below == 5u ? top : s5;
      s6 = below == 6u ? top : s6;
      if (op == kScPushConst) r = in.value;
      else if (op == kScPushField) r = script_pick((code >> 16) & 0xFFu, f0, f1, f2, f3, f4, f5, f6, f7);
      else r = base_score;
      // (a push is not checked, as in the reference: `1 / _score` of an infinite base score is 0.0, not NONE)
    } else {
      if (op == kScNeg) {
        r = -top;
      } else {
        const double a = script_pick(at, s0, s1, s2, s3, s4, s5, s6, s6), b = top;
        if (op == kScAdd) {
          r = a + b;
        } else if (op == kScSub) {
          r = a - b;
        } else if (op == kScMul) {
          r = a * b;
        } else {
          none = none || b == 0.0;
          r = a / b;
        }
      }
      none = none || !isfinite(r);
    }
    top = r;
  }
  const float v = (float)top;  // (a well-formed program ends with one value)
  none = none || !isfinite(v);
  const float score = v * sq.boost;
  none = none || !isfinite(score);
  none_out = none;
  return score;
}

#ifndef SLG_SCRIPT_DEVICE_FUNCTIONS_ONLY  // (a unit that calls script_candidate alone, slg_explain.hip, compiles no second script_kernel)
static __global__ void __launch_bounds__(kScriptThreads) script_kernel(ScriptParams p) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t s = rfl(blockIdx.x * (kScriptThreads / 64) + (threadIdx.x >> 6));
  if (s >= p.c.n_slices) return;
  const RoundQuery rq = load_const(p.c.sq + load_const(p.c.slice_sq + s));
  ClauseSlice sl;
  sl.q = rfl(rq.q);
  sl.seg = rfl(rq.seg);
  const ScriptQuery sq = load_const(p.queries + sl.q);
  const uint32_t n_instrs = rfl(sq.n_instrs);
  if (n_instrs == 0u) return;  // a query without a program is left as it is, bit for bit
  // (slice_cbeg and slice_ccnt were written by the kernels in front of this one, which have finished; this wave's
  //  own store to slice_ccnt[s] comes after its only load of it)
  sl.ccnt = rfl(load_const(p.c.slice_ccnt + s));
  sl.reg = p.c.cand + uniform64(load_const(p.c.slice_cbeg + s));
  sl.kept = sl.rejected = 0u;
  const uint32_t n_fields = rfl(sq.n_fields);
  const ScriptInstr *const prog = p.instrs + rfl(sq.instr_begin);
  for (uint32_t base = 0; base < sl.ccnt; base += 64u) {
    const uint2 c = clause_candidate(sl, base + lane);
    const bool live = c.y != 0xFFFFFFFFu;  // (a dropped entry stays dropped)
    const uint32_t doc = c.y;
    bool none;
    const float score = script_candidate<true>(sq, prog, n_instrs, n_fields, p.cols, p.c.n_segs, sl.seg, doc, live,
                                               fscore_base(c.x), none);
    clause_keep(sl, make_uint2(ordered_score(score), doc), live, live && !none);
  }
  clause_finish(p.c, s, sl, lane);
}
#endif

}  // namespace slg
