// gat_backward_x16.hip — the lane form of the fused GAT backward on fp16 / bf16 grad_out and feat (gat_backward.h): the kernel body of
// gat_backward_kernel.h instantiated on the two 16-bit element types — 3 segment widths, both passes, with and without the leaky factor,
// plain and with dropout: 48 kernels, each serving V = 8 / 4 / 2 / 1 elements per load behind a wave-uniform switch — and the two entry
// points. A translation unit of its own: the fp32 kernels of gat_backward.hip stay exactly what they are. Compiled without packed fp32
// arithmetic; the build fails if an instantiation spills vector registers or uses scratch (Makefile).

#include "gat_backward_kernel.h"

namespace gespmm {

hipError_t launch_gat_backward_el_x16(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, const float* stats,
                                      const void* grad_out, const void* feat, int dtype, float* delta, float* grad_el, int64_t M, int64_t K,
                                      int64_t H, int64_t F, int64_t nnz, float slope, const GatBackwardLaunch& r, const EdgeDropout* drop,
                                      hipStream_t st) {
    const uint16_t *go = static_cast<const uint16_t*>(grad_out), *ft = static_cast<const uint16_t*>(feat);
    if (r.form != kGatBackwardLane) return hipErrorInvalidValue;
    if (dtype == kX16F16)
        return backward_el<kX16F16>(rowptr, colind, el, er, stats, go, ft, delta, grad_el, M, K, H, F, nnz, slope, r.W, r.rpw, r.L, r.V, drop, st);
    if (dtype == kX16Bf16)
        return backward_el<kX16Bf16>(rowptr, colind, el, er, stats, go, ft, delta, grad_el, M, K, H, F, nnz, slope, r.W, r.rpw, r.L, r.V, drop, st);
    return hipErrorInvalidValue;
}

hipError_t launch_gat_backward_er_x16(const int32_t* colptr, const int32_t* rowind, const float* el, const float* er, const float* stats,
                                      const float* delta, const void* grad_out, const void* feat, int dtype, float* grad_er, int64_t M,
                                      int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, const GatBackwardLaunch& r,
                                      const EdgeDropout* drop, hipStream_t st) {
    const uint16_t *go = static_cast<const uint16_t*>(grad_out), *ft = static_cast<const uint16_t*>(feat);
    if (r.form != kGatBackwardLane) return hipErrorInvalidValue;
    if (dtype == kX16F16)
        return backward_er<kX16F16>(colptr, rowind, el, er, stats, delta, go, ft, grad_er, M, K, H, F, nnz, slope, r.W, r.rpw, r.L, r.V, drop, st);
    if (dtype == kX16Bf16)
        return backward_er<kX16Bf16>(colptr, rowind, el, er, stats, delta, go, ft, grad_er, M, K, H, F, nnz, slope, r.W, r.rpw, r.L, r.V, drop, st);
    return hipErrorInvalidValue;
}

}  // namespace gespmm
