// spmm_fused_plan.hip — the fused product on a plan's task tables: the plan-mode instantiations of the two streaming kernels with
// ARGS = FusedSpmmArgs (spmm_stream.h, spmm_fused.h). row_scale is indexed by the C row, i.e. after the plan's permutation.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spmm_fused.h"
#include "spmm_kernels.h"

namespace gespmm {

hipError_t launch_spmm_fused_planned(const FusedSpmmArgs& a, const Geometry& geo, bool segmented, hipStream_t st) {
    if (!a.perm || (segmented ? !a.gtasks : !a.tasks)) return hipErrorInvalidValue;
    return launch_spmm_fused_impl<true>(a, geo, segmented, st);
}

}  // namespace gespmm
