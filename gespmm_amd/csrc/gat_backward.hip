// gat_backward.hip — grad_el and grad_er of a graph attention layer without an edge-sized array (gat_backward.h: contract, lane
// geometry, pinned orders), on fp32 operands: the kernel body of gat_backward_kernel.h (safety rules and the broadcast loads of the
// fixed row are written there) instantiated on float, and the two entry points. A translation unit of its own.

#include "gat_backward_kernel.h"

namespace gespmm {

// The loads are 16 bytes wide when F % 4 == 0 and both operands sit on 16-byte boundaries, 4 bytes wide otherwise.
static int words_per_load(const float* a, const float* b, int64_t F) {
    const bool aligned = (reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) % 16 == 0;
    return (F % 4 == 0 && aligned) ? 4 : 1;
}

hipError_t launch_gat_backward_el(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, const float* stats,
                                  const float* grad_out, const float* feat, float* delta, float* grad_el, int64_t M, int64_t K, int64_t H,
                                  int64_t F, int64_t nnz, float slope, const EdgeSoftmaxLaunch& r, const EdgeDropout* drop, hipStream_t st) {
    return backward_el<0>(rowptr, colind, el, er, stats, grad_out, feat, delta, grad_el, M, K, H, F, nnz, slope, r.W, r.rpw, r.L,
                          words_per_load(grad_out, feat, F), drop, st);
}

hipError_t launch_gat_backward_er(const int32_t* colptr, const int32_t* rowind, const float* el, const float* er, const float* stats,
                                  const float* delta, const float* grad_out, const float* feat, float* grad_er, int64_t M, int64_t K,
                                  int64_t H, int64_t F, int64_t nnz, float slope, const EdgeSoftmaxLaunch& r, const EdgeDropout* drop,
                                  hipStream_t st) {
    return backward_er<0>(colptr, rowind, el, er, stats, delta, grad_out, feat, grad_er, M, K, H, F, nnz, slope, r.W, r.rpw, r.L,
                          words_per_load(grad_out, feat, F), drop, st);
}

}  // namespace gespmm
