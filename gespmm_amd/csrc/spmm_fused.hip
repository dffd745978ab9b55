// spmm_fused.hip — the fused product C = ((A (col_scale . B)) . row_scale) + bias on the caller's CSR: the storage-order
// instantiations of the two streaming kernels with ARGS = FusedSpmmArgs (spmm_stream.h, spmm_fused.h), and the two elementwise
// kernels of the composition route. A translation unit of its own, like spmm_stream_plan.hip: the unfused kernels of
// spmm_kernels.hip stay exactly what they are, and the files compile side by side.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spmm_fused.h"
#include "spmm_kernels.h"

namespace gespmm {

bool fused_geometry_served(const Geometry& geo, bool segmented, bool planned) { return fused_geometry_served_impl(geo, segmented, planned); }

hipError_t launch_spmm_fused(const FusedSpmmArgs& a, const Geometry& geo, bool segmented, hipStream_t st) {
    if (a.tasks || a.gtasks) return launch_spmm_fused_planned(a, geo, segmented, st);
    return launch_spmm_fused_impl<false>(a, geo, segmented, st);
}

// ----------------------------------------------------------------------------- composition route: the two elementwise passes
//
// One lane per VEC consecutive floats of a row, rows dealt to the grid's y dimension in steps: the row's scale is one scalar-like
// load per lane (same address across the lanes of a row), the row itself streams through once. VEC = 4 (dwordx4) where the width
// and both pointers allow it, else 1.

template <int VEC>
__global__ __launch_bounds__(256) void scale_rows_kernel(const float* __restrict__ B, const float* __restrict__ col_scale,
                                                         float* __restrict__ Bs, int64_t K, int64_t N) {
    const int64_t per_row = N / VEC;
    const int64_t total = K * per_row;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = i / per_row;
        const float s = col_scale[k];
        float v[VEC];
        load_vec<VEC>(v, reinterpret_cast<const char*>(B + i * VEC));
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[j] = __fmul_rn(v[j], s);
        store_vec<VEC, false>(Bs + i * VEC, v);
    }
}

template <int VEC>
__global__ __launch_bounds__(256) void scale_bias_inplace_kernel(float* __restrict__ C, const float* __restrict__ row_scale,
                                                                 const float* __restrict__ bias, int64_t M, int64_t N) {
    const int64_t per_row = N / VEC;
    const int64_t total = M * per_row;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / per_row;
        const int64_t c = (i - r * per_row) * VEC;
        float v[VEC];
        load_vec<VEC>(v, reinterpret_cast<const char*>(C + i * VEC));
        if (row_scale != nullptr) {
            const float s = row_scale[r];
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[j] = __fmul_rn(v[j], s);
        }
        if (bias != nullptr) {
            float b[VEC];
            load_vec<VEC>(b, reinterpret_cast<const char*>(bias + c));
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[j] = __fadd_rn(v[j], b[j]);
        }
        store_vec<VEC, false>(C + i * VEC, v);
    }
}

static inline bool all_aligned16(const void* p, const void* q, const void* r) {
    return ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(r)) & 15) == 0;
}

static inline unsigned elementwise_blocks(int64_t items) {
    int64_t b = (items + 255) / 256;
    const int64_t cap = 256 * 32;  // a few workgroups per CU, grid-stride beyond
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

hipError_t launch_scale_rows(const float* B, const float* col_scale, float* Bs, int64_t K, int64_t N, hipStream_t st) {
    if (K <= 0 || N <= 0) return hipSuccess;
    if (N % 4 == 0 && all_aligned16(B, Bs, nullptr))
        hipLaunchKernelGGL(scale_rows_kernel<4>, dim3(elementwise_blocks(K * (N / 4))), dim3(256), 0, st, B, col_scale, Bs, K, N);
    else
        hipLaunchKernelGGL(scale_rows_kernel<1>, dim3(elementwise_blocks(K * N)), dim3(256), 0, st, B, col_scale, Bs, K, N);
    return hipGetLastError();
}

hipError_t launch_scale_bias_inplace(float* C, const float* row_scale, const float* bias, int64_t M, int64_t N, hipStream_t st) {
    if (M <= 0 || N <= 0 || (!row_scale && !bias)) return hipSuccess;
    if (N % 4 == 0 && all_aligned16(C, bias, nullptr))
        hipLaunchKernelGGL(scale_bias_inplace_kernel<4>, dim3(elementwise_blocks(M * (N / 4))), dim3(256), 0, st, C, row_scale, bias, M, N);
    else
        hipLaunchKernelGGL(scale_bias_inplace_kernel<1>, dim3(elementwise_blocks(M * N)), dim3(256), 0, st, C, row_scale, bias, M, N);
    return hipGetLastError();
}

}  // namespace gespmm
