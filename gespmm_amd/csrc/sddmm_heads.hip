// sddmm_heads.hip — the multi-head SDDMM on fp32 operands (gfx950): the kernel of sddmm_heads.h instantiated on the SddmmF32 trait,
// and the two small kernels its routes need around it.
//
//     out[e H + h] = sum_{j < F} D1[row(e), h F + j] * D2[col(e), h F + j]        (pattern order, head-minor)

#define GESPMM_SDDMM_HEADS_KERNELS
#include "sddmm_heads.h"

#include "sddmm_f32.h"

namespace gespmm {

hipError_t launch_sddmm_heads(const int32_t* rows, const int32_t* colind, const float* D1, const float* D2, float* out, int64_t M,
                              int64_t nnz, int64_t H, int64_t F, const SddmmHeadsLaunch& r, hipStream_t st) {
    return launch_sddmm_heads_op<SddmmF32>(rows, colind, D1, D2, out, M, nnz, H, F, r, st);
}

// One atomic per wavefront: lanes take a grid-stride maximum, the wavefront folds it with an xor butterfly.
__global__ __launch_bounds__(256) void max_index_kernel(const int32_t* __restrict__ idx, int64_t n, int32_t* __restrict__ result) {
    int m = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) m = idx[i] > m ? idx[i] : m;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const int o = __shfl_xor(m, s, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(result, m);
}

hipError_t launch_max_index(const int32_t* idx, int64_t n, int32_t* result, hipStream_t st) {
    hipError_t e = hipMemsetAsync(result, 0, sizeof(int32_t), st);
    if (e != hipSuccess || n <= 0) return e;
    int64_t b = (n + 255) / 256;
    if (b > 2048) b = 2048;
    hipLaunchKernelGGL(max_index_kernel, dim3((unsigned)b), dim3(256), 0, st, idx, n, result);
    return hipGetLastError();
}

// Consecutive threads copy consecutive words of src; the H words of an edge land next to each other in dst.
__global__ __launch_bounds__(256) void scatter_heads_kernel(const float* __restrict__ src, const int32_t* __restrict__ dst_index,
                                                            float* __restrict__ dst, int64_t n, int H) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = i / H;
        const int h = (int)(i - p * H);
        dst[(size_t)dst_index[p] * (size_t)H + h] = src[i];
    }
}

hipError_t launch_scatter_heads(const float* src, const int32_t* dst_index, float* dst, int64_t nnz, int64_t H, hipStream_t st) {
    const int64_t n = nnz * H;
    if (n <= 0) return hipSuccess;
    int64_t b = (n + 255) / 256;
    if (b > 256 * 32) b = 256 * 32;
    hipLaunchKernelGGL(scatter_heads_kernel, dim3((unsigned)b), dim3(256), 0, st, src, dst_index, dst, n, (int)H);
    return hipGetLastError();
}

}  // namespace gespmm
