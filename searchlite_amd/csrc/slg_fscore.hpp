// slg_fscore.hpp — function_score at the root of the score tree (slg_batch_prepare_fscore): the reference's
// evaluate_compiled_score for a FunctionScore node (api/reader.rs:491-548; query/score_functions.rs) as one
// kernel between the scoring kernel and the select.  The semantics in full: include/searchlite_gpu.h.  In short,
// per candidate:
//   every function gives a value (f32) or none: weight -> w; field_value_factor -> modifier(first value of the
//   column, or missing, times (double)factor), none when the product or the result is not finite; decay -> none
//   without a value, else exp pow(decay, norm), gauss pow(decay, norm * norm), linear max((1 - norm) * (1 - decay)
//   + decay, 0) with norm = max(|v - origin| - offset, 0) / scale; a function whose filter rejects the doc: none.
//   All in f64, one operation at a time (the unit is built with -ffp-contract=off and without fast-math).
//   fs = the present values folded left to right in f32 by the score mode (avg: the sum over their number);
//   eff = base, but 1.0 when |base| <= FLT_EPSILON and a value is present; combined = eff without a value, else
//   boost_mode(eff, fs); then min(combined, max_boost), then the doc is dropped when combined < min_score, then
//   combined *= boost.  max / min are fmaxf / fminf (a NaN operand loses, as Rust's f32::max / min).
//
// A function_score batch runs in candidates mode: the scoring kernel leaves every doc of the scored lists, with
// its exact score, in the region (slice_cbeg[s], slice_ccnt[s]) of its slice.  fscore_kernel rewrites every
// candidate as {ordered key of the new score, doc}, writes the survivors back to the front of the same region and
// stores the new slice_ccnt — the format the selects read, so none of them changes.
//
// Shape: the clause filters' (slg_clause.hpp) — one wave per slice, four per workgroup, one candidate per lane,
// 64 per chunk; clause_candidate, clause_keep and clause_finish are theirs, with the invariant of the in-place
// store stated there.  The query's record and its function row are wave-uniform and read through the constant
// address space (scalar loads); so are the column and bitmap addresses of the slice's segment.  Per candidate and
// function the vector loads are: one word of the filter's bitmap, offsets[doc] and offsets[doc + 1] (none when the
// column is stored without offsets), values[first].
//
// FULL = false compiles the kernel without ln / log1p / log2 / pow (the device library's f64 forms are the
// register-heavy part): the host launches it for batches whose functions need none of them.
#pragma once

#include "slg_clause.hpp"

namespace slg {

constexpr int kFscoreThreads = 256;  // four waves = four slices per workgroup

// the values of searchlite_gpu.h's enums (checked in slg_fscore.hip)
constexpr uint32_t kFsWeight = 0, kFsFieldValue = 1, kFsDecay = 2;
constexpr uint32_t kFsModNone = 0, kFsModLog = 1, kFsModLog1p = 2, kFsModLog2p = 3, kFsModSqrt = 4, kFsModReciprocal = 5;
constexpr uint32_t kFsDecayExp = 0, kFsDecayGauss = 1, kFsDecayLinear = 2;
constexpr uint32_t kFsSum = 0, kFsMultiply = 1, kFsMax = 2, kFsMin = 3, kFsAvg = 4;
constexpr uint32_t kFsBoostMultiply = 0, kFsBoostSum = 1, kFsBoostReplace = 2, kFsBoostMax = 3, kFsBoostMin = 4;
constexpr uint32_t kFsHasMaxBoost = 1, kFsHasMinScore = 2;

struct FscoreParams {
  BoolFilterParams c;            // the slices, the candidates and q_scored (queries and terms: unused, null)
  const FscoreQuery *queries;    // [nq]
  const FscoreFn *fns;           // the functions of all queries
  const ColumnDev *cols;         // [fields of the batch][n_segs]
  const uint32_t *const *filters;  // [filters of the batch][n_segs] reject bitmaps (bit set: the filter rejects)
};

// the f32 an ordered key stands for (ordered_score's inverse)
__device__ __forceinline__ float fscore_base(uint32_t key) {
  return __int_as_float((int32_t)((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key));
}

// apply_modifier (score_functions.rs:194-233), its branch conditions as they stand there
template <bool FULL>
__device__ __forceinline__ double fscore_modifier(double x, uint32_t mod) {
  if (mod == kFsModSqrt) return x < 0.0 ? 0.0 : sqrt(x);
  if (mod == kFsModReciprocal) return x == 0.0 ? 0.0 : 1.0 / x;
  if constexpr (FULL) {
    if (mod == kFsModLog) return x <= 0.0 ? 0.0 : log(x);
    if (mod == kFsModLog1p) return x <= -1.0 ? 0.0 : log1p(x);
    if (mod == kFsModLog2p) return x <= -1.0 ? 0.0 : log2(x + 1.0);
  }
  return x;
}

// A value that is wave-uniform where one wave works on one segment (UNI: the kernels between scoring and select, which
// keep it in scalar registers), and per lane where a lane's rows lie in any segment (explain_kernel, slg_explain.hpp)
template <bool UNI>
__device__ __forceinline__ uint32_t fscore_u32(uint32_t v) {
  if constexpr (UNI) return rfl(v);
  else return v;
}
template <bool UNI>
__device__ __forceinline__ uint64_t fscore_u64(uint64_t v) {
  if constexpr (UNI) return uniform64(v);
  else return v;
}

// One candidate through the functions of its query: the new score (boost applied) and, in `accept`, whether the doc
// stays (live, and not below min_score).  row: the query's functions; n_fns, score_mode, boost_mode, flags: the
// query's, wave-uniform.  emit(kinds, field id, value) is called, in request order, for every function that gives the
// doc a value (the entries of an explanation; fscore_kernel passes a callable that does nothing).
template <bool FULL, bool UNI, typename Emit>
__device__ __forceinline__ float fscore_candidate(const FscoreQuery &fq, const FscoreFn *const row, const uint32_t n_fns,
                                                  const uint32_t score_mode, const uint32_t boost_mode, const uint32_t flags,
                                                  const ColumnDev *const cols, const uint32_t *const *const filters,
                                                  const uint32_t n_segs, const uint32_t seg, const uint32_t doc,
                                                  const bool live, const float base_score, bool &accept, Emit emit) {
  float fs = 0.0f;
  uint32_t present = 0u;
  for (uint32_t f = 0; f < n_fns; f++) {
    const FscoreFn fn = load_const(row + f);
    const uint32_t kinds = rfl(fn.kinds);
    const uint32_t kind = kinds & 0xFFu;
    bool has = live;
    const uint32_t flt = rfl(fn.filter);
    if (flt != 0u) {
      typedef const __attribute__((address_space(1))) uint32_t *gu32_t;
      const uint64_t a = fscore_u64<UNI>((uint64_t)(uintptr_t)load_const(filters + ((size_t)(flt - 1u) * n_segs + seg)));
      uint32_t w = 0u;
      if (has && a != 0ull) w = ((gu32_t)(uintptr_t)a)[doc >> 5];  // (a live doc is below the segment's n_docs)
      has = has && ((w >> (doc & 31u)) & 1u) == 0u;
    }
    double v = 0.0;
    if (kind != kFsWeight) {  // the doc's first value of the column
      typedef const __attribute__((address_space(1))) uint32_t *gu32_t;
      typedef const __attribute__((address_space(1))) double *gf64_t;
      const ColumnDev col = load_const(cols + ((size_t)rfl(fn.col) * n_segs + seg));
      const uint64_t offs = fscore_u64<UNI>((uint64_t)(uintptr_t)col.offs), vals = fscore_u64<UNI>((uint64_t)(uintptr_t)col.vals);
      uint32_t first = doc, end = doc + 1u;
      if (offs != 0ull && has) {
        first = ((gu32_t)(uintptr_t)offs)[doc];
        end = ((gu32_t)(uintptr_t)offs)[doc + 1u];
      }
      const bool valued = has && first < end;
      if (valued) v = ((gf64_t)(uintptr_t)vals)[first];
      if (kind == kFsFieldValue) {
        const double raw = valued ? v : fn.missing;
        const double scaled = raw * (double)fn.weight;
        v = fscore_modifier<FULL>(scaled, (kinds >> 8) & 0xFFu);
        has = has && isfinite(scaled) && isfinite(v);
      } else {
        const double distance = fabs(v - fn.origin) - fn.offset;
        const double norm = fmax(distance, 0.0) / fn.scale;
        const uint32_t dfn = (kinds >> 16) & 0xFFu;
        if (dfn == kFsDecayLinear) {
          v = fmax((1.0 - norm) * (1.0 - fn.decay) + fn.decay, 0.0);
        } else {
          if constexpr (FULL) v = pow(fn.decay, dfn == kFsDecayGauss ? norm * norm : norm);
        }
        has = valued && isfinite(v);
      }
    }
    const float val = kind == kFsWeight ? fn.weight : (float)v;
    if (has) {
      float next;
      if (score_mode == kFsMultiply) next = fs * val;
      else if (score_mode == kFsMax) next = fmaxf(fs, val);
      else if (score_mode == kFsMin) next = fminf(fs, val);
      else next = fs + val;
      fs = present == 0u ? val : next;
      present++;
      emit(kinds, fn.field, val);
    }
  }
  float eff = base_score;
  if (present != 0u && fabsf(base_score) <= 1.1920929e-7f) eff = 1.0f;  // (f32::EPSILON)
  float combined = eff;
  if (present != 0u) {
    if (score_mode == kFsAvg) fs = fs / (float)present;
    if (boost_mode == kFsBoostMultiply) combined = eff * fs;
    else if (boost_mode == kFsBoostSum) combined = eff + fs;
    else if (boost_mode == kFsBoostReplace) combined = fs;
    else if (boost_mode == kFsBoostMax) combined = fmaxf(eff, fs);
    else combined = fminf(eff, fs);
  }
  if (flags & kFsHasMaxBoost) combined = fminf(combined, fq.max_boost);
  accept = live && !((flags & kFsHasMinScore) != 0u && combined < fq.min_score);
  combined *= fq.boost;
  return combined;
}

template <bool FULL>
static __global__ void __launch_bounds__(kFscoreThreads) fscore_kernel(FscoreParams p) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t s = rfl(blockIdx.x * (kFscoreThreads / 64) + (threadIdx.x >> 6));
  if (s >= p.c.n_slices) return;
  const RoundQuery rq = load_const(p.c.sq + load_const(p.c.slice_sq + s));
  ClauseSlice sl;
  sl.q = rfl(rq.q);
  sl.seg = rfl(rq.seg);
  const FscoreQuery fq = load_const(p.queries + sl.q);
  if (rfl(fq.work) == 0u) return;  // a query without work is left as it is, bit for bit
  // (slice_cbeg and slice_ccnt were written by the scoring kernel, which has finished; this wave's own store to
  //  slice_ccnt[s] comes after its only load of it)
  sl.ccnt = rfl(load_const(p.c.slice_ccnt + s));
  sl.reg = p.c.cand + uniform64(load_const(p.c.slice_cbeg + s));
  sl.kept = sl.rejected = 0u;
  const uint32_t n_fns = rfl(fq.n_fns), modes = rfl(fq.modes);
  const uint32_t score_mode = modes & 0xFFu, boost_mode = (modes >> 8) & 0xFFu, flags = (modes >> 16) & 0xFFu;
  const FscoreFn *const row = p.fns + rfl(fq.fn_begin);
  for (uint32_t base = 0; base < sl.ccnt; base += 64u) {
    const uint2 c = clause_candidate(sl, base + lane);
    const bool live = c.y != 0xFFFFFFFFu;  // (a dropped entry stays dropped)
    const uint32_t doc = c.y;
    bool accept;
    const float combined = fscore_candidate<FULL, true>(fq, row, n_fns, score_mode, boost_mode, flags, p.cols, p.filters,
                                                        p.c.n_segs, sl.seg, doc, live, fscore_base(c.x), accept,
                                                        [](uint32_t, int32_t, float) {});
    clause_keep(sl, make_uint2(ordered_score(combined), doc), live, accept);
  }
  clause_finish(p.c, s, sl, lane);
}

}  // namespace slg
