// spmm_x16_plan.hip — 16-bit dense operands on a plan's task tables: the plan-mode instantiations of the two streaming kernels with
// ARGS = HalfSpmmArgs<DT> (spmm_stream.h, spmm_x16.h). Row i of the plan's copy is written to C row perm[i], as in the fp32 kernels.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spmm_kernels.h"
#include "spmm_x16.h"

namespace gespmm {

hipError_t launch_spmm_x16_planned(const SpmmArgs& a, int dtype, const Geometry& geo, bool segmented, hipStream_t st) {
    if (!a.perm || (segmented ? !a.gtasks : !a.tasks)) return hipErrorInvalidValue;
    return launch_spmm_x16_impl<true>(a, dtype, geo, segmented, st);
}

}  // namespace gespmm
