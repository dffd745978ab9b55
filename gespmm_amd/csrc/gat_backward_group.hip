// gat_backward_group.hip — the group form of the fused GAT backward on fp32 operands: the kernel body of gat_backward_group_kernel.h
// instantiated on float, and the two entry points. A translation unit of its own.

#include "gat_backward_group_kernel.h"

namespace gespmm {

hipError_t launch_gat_backward_group_el(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, const float* stats,
                                        const float* grad_out, const float* feat, float* delta, float* grad_el, int64_t M, int64_t K,
                                        int64_t H, int64_t F, int64_t nnz, float slope, const GatBackwardLaunch& r, const EdgeDropout* drop,
                                        hipStream_t st) {
    return group_el<0>(rowptr, colind, el, er, stats, grad_out, feat, delta, grad_el, M, K, H, F, nnz, slope, r, drop, st);
}

hipError_t launch_gat_backward_group_er(const int32_t* colptr, const int32_t* rowind, const float* el, const float* er, const float* stats,
                                        const float* delta, const float* grad_out, const float* feat, float* grad_er, int64_t M, int64_t K,
                                        int64_t H, int64_t F, int64_t nnz, float slope, const GatBackwardLaunch& r, const EdgeDropout* drop,
                                        hipStream_t st) {
    return group_er<0>(colptr, rowind, el, er, stats, delta, grad_out, feat, grad_er, M, K, H, F, nnz, slope, r, drop, st);
}

}  // namespace gespmm
