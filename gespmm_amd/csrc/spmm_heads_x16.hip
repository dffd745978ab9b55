// spmm_heads_x16.hip — the multi-head product on 16-bit dense operands (gespmm_csr_spmm_heads_x16: IEEE fp16 / bfloat16 B and C, fp32
// weights, fp32 sums rounded once at the store): the kernel body of spmm_heads_kernel.h instantiated on the two 16-bit element types,
// and its launch table. A translation unit of its own: the fp32 kernels of spmm_heads.hip stay exactly what they are.
//
// The kernels work in 32-bit words, so a geometry here is the one select.cpp resolves for the width in WORDS, H F / 2, with V words per
// lane and strip and V | F / 2 (a lane's vector stays inside one head). Storage order only — there is no plan form of this product —
// so the table is the stateless part of spmm_heads.hip's: 11 geometries, for fp16 and bf16.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spmm_device.h"
#include "spmm_heads.h"
#include "spmm_heads_kernel.h"

namespace gespmm {

template <int DT, int V, int S, int W>
static hipError_t launch_heads_x16(const HeadsArgs& a, int rpw, hipStream_t st) {
    constexpr int U = (V * S >= 8) ? 4 : 8;  // gather depth in words, as the 16-bit streaming kernels (spmm_x16.h)
    HeadsArgs args;
    int64_t nitems = 0;
    if (!heads_launch_shape<V, S, W, false>(a, rpw, &args, &nitems)) return nitems <= 0 ? hipSuccess : hipErrorInvalidConfiguration;
    hipLaunchKernelGGL((spmm_heads_kernel_t<DT, V, S, W, U, false>), dim3((unsigned)nitems), dim3(kThreads), 0, st, args);
    return hipGetLastError();
}

template <int DT>
static hipError_t launch_heads_x16_geometry(const HeadsArgs& a, const Geometry& g, hipStream_t st) {
#define GESPMM_HEADS_X16(V_, S_, W_) \
    if (g.vec == V_ && g.strips == S_ && g.group == W_) return launch_heads_x16<DT, V_, S_, W_>(a, g.rows_per_wave, st);
    GESPMM_HEADS_X16(1, 1, 4)
    GESPMM_HEADS_X16(1, 1, 8)
    GESPMM_HEADS_X16(1, 1, 16)
    GESPMM_HEADS_X16(1, 1, 32)
    GESPMM_HEADS_X16(1, 1, 64)
    GESPMM_HEADS_X16(4, 1, 32)
    GESPMM_HEADS_X16(4, 1, 64)
    GESPMM_HEADS_X16(4, 2, 64)
    GESPMM_HEADS_X16(2, 1, 64)
    GESPMM_HEADS_X16(2, 2, 64)
    GESPMM_HEADS_X16(1, 2, 64)
#undef GESPMM_HEADS_X16
    return hipErrorInvalidValue;
}

// `a` is the launch in WORDS: a.B / a.C the 16-bit arrays, a.N = H F / 2, a.F = F / 2 (spmm_heads.h).
hipError_t launch_spmm_heads_x16(const HeadsArgs& a, int dtype, const Geometry& geo, hipStream_t st) {
    if (a.tasks != nullptr || a.H < 2 || a.H > kHeadsMax || a.F < 1 || a.N != a.H * a.F || a.F % geo.vec != 0) return hipErrorInvalidValue;
    // (a.val / a.colind / a.B may be NULL when the matrix has no entries: every load of them sits under a position compare)
    if (!heads_geometry_served(geo, false)) return hipErrorInvalidValue;
    if (dtype == kX16F16) return launch_heads_x16_geometry<kX16F16>(a, geo, st);
    if (dtype == kX16Bf16) return launch_heads_x16_geometry<kX16Bf16>(a, geo, st);
    return hipErrorInvalidValue;
}

// ----------------------------------------------------------------------------- composition route of the 16-bit multi-head SDDMM
//
// The 2-byte forms of launch_heads_slice / launch_heads_unslice: dst[r, 0:width] = src[r, off:off+width] on 16-bit elements.

__global__ __launch_bounds__(256) void heads_slice_x16_kernel(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, int64_t rows,
                                                              int64_t stride, int64_t off, int64_t width) {
    const int64_t n = rows * width;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / width, j = i - r * width;
        dst[i] = src[r * stride + off + j];
    }
}

hipError_t launch_heads_slice_x16(const void* src, void* dst, int64_t rows, int64_t stride, int64_t off, int64_t width, hipStream_t st) {
    if (rows <= 0 || width <= 0) return hipSuccess;
    int64_t b = (rows * width + 255) / 256;
    const int64_t cap = 256 * 32;  // a few workgroups per CU, grid-stride beyond
    hipLaunchKernelGGL(heads_slice_x16_kernel, dim3((unsigned)(b > cap ? cap : b)), dim3(256), 0, st, static_cast<const uint16_t*>(src),
                       static_cast<uint16_t*>(dst), rows, stride, off, width);
    return hipGetLastError();
}

}  // namespace gespmm
