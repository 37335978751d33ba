// slg_score_inst.hip — one translation unit per top-k register width (SLG_INST_KREGS), so the
// scoring-kernel instantiations compile in parallel.  slg_batch.hip calls
// slg::launch_score_kregs<N>() declared below.
#include <hip/hip_runtime.h>

#include "slg_score.hpp"
#include "slg_score_uni4.hpp"
#include "slg_score_multi.hpp"

#ifndef SLG_INST_KREGS
#error "compile with -DSLG_INST_KREGS={1,2,4,8,16}"
#endif

namespace slg {

template <int KREGS>
void launch_score_kregs(const RoundScoreParams &sp, int kind, hipStream_t st);

// Waves are independent in both kernels (no workgroup barrier anywhere), so workgroups are ONE
// wave: a finished wave frees its wave slot and its LDS at once.  One wave per slice.

// the few-term kernel (slg_score_uni4.hpp): <= 4 (ML 4) or 5..8 (ML 8) lists per sub-query
// (static: every unit has its own, for its own SLG_INST_KREGS)
template <int ML, bool PLAN>
static void launch_uniform4(const RoundScoreParams &sp, hipStream_t st) {
  hipLaunchKernelGGL((score_uniform4_kernel<SLG_INST_KREGS, ML, PLAN>), dim3(sp.n_slices), dim3(64),
                     u4_wave_lds(SLG_INST_KREGS, ML, u4_filter_words(ML)), st, sp);
}

template <>
void launch_score_kregs<SLG_INST_KREGS>(const RoundScoreParams &sp, int kind, hipStream_t st) {
  if (kind >= 6 && kind <= 9) {  // few-term kernel: 6 / 7 <= 4 / 5..8 lists; 8 / 9 the same with score plans
    const bool ml8 = (kind & 1) != 0, plan = kind >= 8;  // (plans: flat Sum / DisMax over multi-term leaves)
    if (plan)
      ml8 ? launch_uniform4<8, true>(sp, st) : launch_uniform4<4, true>(sp, st);
    else
      ml8 ? launch_uniform4<8, false>(sp, st) : launch_uniform4<4, false>(sp, st);
    return;
  }
  // many lists: slots of one list each, 8 at a time (slg_score_multi.hpp)
  const size_t lds = (size_t)multi_wave_lds(SLG_INST_KREGS) + (size_t)sp.plan_batch * kMultiPlanLds;
  if (sp.plan_batch == 4)  // score trees of more than two levels
    hipLaunchKernelGGL((score_multi_kernel<SLG_INST_KREGS, 4>), dim3(sp.n_slices), dim3(64), lds, st, sp);
  else if (sp.plan_batch == 2)  // two-level score plans
    hipLaunchKernelGGL((score_multi_kernel<SLG_INST_KREGS, 3>), dim3(sp.n_slices), dim3(64), lds, st, sp);
  else if (sp.plan_batch)  // score plans (never together with pruning)
    hipLaunchKernelGGL((score_multi_kernel<SLG_INST_KREGS, 2>), dim3(sp.n_slices), dim3(64), lds, st, sp);
  else if (kind == 3)  // pruning-classified batch
    hipLaunchKernelGGL((score_multi_kernel<SLG_INST_KREGS, 1>), dim3(sp.n_slices), dim3(64), lds, st, sp);
  else
    hipLaunchKernelGGL((score_multi_kernel<SLG_INST_KREGS, 0>), dim3(sp.n_slices), dim3(64), lds, st, sp);
}

}  // namespace slg
