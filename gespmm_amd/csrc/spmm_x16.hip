// spmm_x16.hip — 16-bit dense operands (IEEE fp16 / bfloat16 B and C, fp32 sum rounded once at the store) on the caller's CSR: the
// storage-order instantiations of the two streaming kernels with ARGS = HalfSpmmArgs<DT> (spmm_stream.h, spmm_x16.h), and the two
// elementwise kernels of the composition route. A translation unit of its own, like spmm_fused.hip: the fp32 kernels stay exactly
// what they are.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spmm_kernels.h"
#include "spmm_x16.h"

namespace gespmm {

bool x16_geometry_served(const Geometry& geo, bool segmented, bool planned) { return x16_geometry_served_impl(geo, segmented, planned); }

hipError_t launch_spmm_x16(const SpmmArgs& a, int dtype, const Geometry& geo, bool segmented, hipStream_t st) {
    if (a.tasks || a.gtasks) return launch_spmm_x16_planned(a, dtype, geo, segmented, st);
    return launch_spmm_x16_impl<false>(a, dtype, geo, segmented, st);
}

// ----------------------------------------------------------------------------- composition route: widen and narrow
//
// Plain streaming passes over K x N / M x N elements, grid-stride. PAIRS = true: both arrays allow 32-bit accesses on the 16-bit side
// (address and element count even) and a lane moves one word = two elements (8 bytes of fp32); else one element per lane — operands that
// are only 2-byte aligned, odd counts. The arithmetic is widen_x16 / narrow_x16 of spmm_device.h: what the kernels above do in registers.

template <int DT, bool PAIRS>
__global__ __launch_bounds__(256) void widen_x16_kernel(const uint16_t* __restrict__ src, float* __restrict__ dst, int64_t n) {
    const int64_t items = PAIRS ? n / 2 : n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        if constexpr (PAIRS) {
            float lo, hi;
            widen_x16<DT>(reinterpret_cast<const float*>(src)[i], lo, hi);
            const float v[2] = {lo, hi};
            store_vec<2, false>(dst + 2 * i, v);
        } else {
            float lo, hi;
            widen_x16<DT>(__uint_as_float((uint32_t)src[i]), lo, hi);
            dst[i] = lo;
        }
    }
}

template <int DT, bool PAIRS>
__global__ __launch_bounds__(256) void narrow_x16_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, int64_t n) {
    const int64_t items = PAIRS ? n / 2 : n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        if constexpr (PAIRS) {
            float v[2];
            load_vec<2>(v, reinterpret_cast<const char*>(src + 2 * i));
            reinterpret_cast<uint32_t*>(dst)[i] = narrow_x16<DT>(v[0]) | (narrow_x16<DT>(v[1]) << 16);
        } else {
            dst[i] = (uint16_t)narrow_x16<DT>(src[i]);
        }
    }
}

static inline unsigned x16_elementwise_blocks(int64_t items) {
    int64_t b = (items + 255) / 256;
    const int64_t cap = 256 * 32;  // a few workgroups per CU, grid-stride beyond
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

hipError_t launch_widen_x16(const void* src, float* dst, int dtype, int64_t n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (dtype != kX16F16 && dtype != kX16Bf16) return hipErrorInvalidValue;
    const uint16_t* s = static_cast<const uint16_t*>(src);
    const bool pairs = n % 2 == 0 && reinterpret_cast<uintptr_t>(src) % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 8 == 0;
    const dim3 grid(x16_elementwise_blocks(pairs ? n / 2 : n)), block(256);
    if (dtype == kX16F16) {
        if (pairs) hipLaunchKernelGGL((widen_x16_kernel<kX16F16, true>), grid, block, 0, st, s, dst, n);
        else hipLaunchKernelGGL((widen_x16_kernel<kX16F16, false>), grid, block, 0, st, s, dst, n);
    } else {
        if (pairs) hipLaunchKernelGGL((widen_x16_kernel<kX16Bf16, true>), grid, block, 0, st, s, dst, n);
        else hipLaunchKernelGGL((widen_x16_kernel<kX16Bf16, false>), grid, block, 0, st, s, dst, n);
    }
    return hipGetLastError();
}

hipError_t launch_narrow_x16(const float* src, void* dst, int dtype, int64_t n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (dtype != kX16F16 && dtype != kX16Bf16) return hipErrorInvalidValue;
    uint16_t* d = static_cast<uint16_t*>(dst);
    const bool pairs = n % 2 == 0 && reinterpret_cast<uintptr_t>(dst) % 4 == 0 && reinterpret_cast<uintptr_t>(src) % 8 == 0;
    const dim3 grid(x16_elementwise_blocks(pairs ? n / 2 : n)), block(256);
    if (dtype == kX16F16) {
        if (pairs) hipLaunchKernelGGL((narrow_x16_kernel<kX16F16, true>), grid, block, 0, st, src, d, n);
        else hipLaunchKernelGGL((narrow_x16_kernel<kX16F16, false>), grid, block, 0, st, src, d, n);
    } else {
        if (pairs) hipLaunchKernelGGL((narrow_x16_kernel<kX16Bf16, true>), grid, block, 0, st, src, d, n);
        else hipLaunchKernelGGL((narrow_x16_kernel<kX16Bf16, false>), grid, block, 0, st, src, d, n);
    }
    return hipGetLastError();
}

}  // namespace gespmm
