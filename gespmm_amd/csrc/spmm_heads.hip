// spmm_heads.hip — the multi-head product (spmm_heads.h): the batch-stream kernel of spmm_stream.h at width N = H F with H weights per
// CSR entry (body: spmm_heads_kernel.h), its fp32 launch table (storage order and a plan's task tables), and the copies of the composition route and of a plan's
// per-call weight permutation. A translation unit of its own: the kernels of spmm_stream.h stay exactly what they are.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spmm_device.h"
#include "spmm_heads.h"
#include "spmm_heads_kernel.h"

namespace gespmm {

// ----------------------------------------------------------------------------- multi-head batch-stream kernel
//
// The body — and what it does — is spmm_heads_kernel.h's, on fp32 elements (DT = 0); the 16-bit forms are spmm_heads_x16.hip's.

template <int V, int S, int W, int U, bool PLANNED>
constexpr auto spmm_heads_kernel = spmm_heads_kernel_t<0, V, S, W, U, PLANNED>;

// ----------------------------------------------------------------------------- launch table

template <int V, int S, int W, bool PLANNED>
static hipError_t launch_heads(const HeadsArgs& a, int rpw, hipStream_t st) {
    constexpr int U = (V * S >= 8) ? 4 : 8;  // gather depth, as launch_stream (spmm_stream.h) without the shallow knob
    HeadsArgs args;
    int64_t nitems = 0;
    if (!heads_launch_shape<V, S, W, PLANNED>(a, rpw, &args, &nitems)) return nitems <= 0 ? hipSuccess : hipErrorInvalidConfiguration;
    hipLaunchKernelGGL((spmm_heads_kernel<V, S, W, U, PLANNED>), dim3((unsigned)nitems), dim3(kThreads), 0, st, args);
    return hipGetLastError();
}

template <bool PLANNED>
static hipError_t launch_heads_geometry(const HeadsArgs& a, const Geometry& g, hipStream_t st) {
#define GESPMM_HEADS(V_, S_, W_) \
    if (g.vec == V_ && g.strips == S_ && g.group == W_) return launch_heads<V_, S_, W_, PLANNED>(a, g.rows_per_wave, st);
    GESPMM_HEADS(1, 1, 4)
    GESPMM_HEADS(1, 1, 8)
    GESPMM_HEADS(1, 1, 16)
    GESPMM_HEADS(1, 1, 32)
    GESPMM_HEADS(1, 1, 64)
    GESPMM_HEADS(4, 1, 32)
    GESPMM_HEADS(4, 1, 64)
    GESPMM_HEADS(4, 2, 64)
    GESPMM_HEADS(2, 1, 64)
    GESPMM_HEADS(2, 2, 64)
    GESPMM_HEADS(1, 2, 64)
    if constexpr (PLANNED) {
        GESPMM_HEADS(4, 1, 4)
        GESPMM_HEADS(4, 1, 8)
        GESPMM_HEADS(4, 1, 16)
    }
#undef GESPMM_HEADS
    return hipErrorInvalidValue;
}

hipError_t launch_spmm_heads(const HeadsArgs& a, const Geometry& geo, hipStream_t st) {
    const bool planned = a.tasks != nullptr;
    if (a.H < 2 || a.H > kHeadsMax || a.F < 1 || a.N != a.H * a.F || a.F % geo.vec != 0) return hipErrorInvalidValue;
    // (a.val / a.colind / a.B may be NULL when the matrix has no entries: every load of them sits under a position compare)
    if (!heads_geometry_served(geo, planned)) return hipErrorInvalidValue;
    if (planned) {
        if (!a.perm) return hipErrorInvalidValue;
        return launch_heads_geometry<true>(a, geo, st);
    }
    return launch_heads_geometry<false>(a, geo, st);
}

// ----------------------------------------------------------------------------- composition route and plan: plain copies, grid-stride

template <bool INVERSE>
__global__ __launch_bounds__(256) void heads_slice_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t rows,
                                                          int64_t stride, int64_t off, int64_t width) {
    const int64_t n = rows * width;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / width, j = i - r * width;
        if constexpr (INVERSE) dst[r * stride + off + j] = src[i];
        else dst[i] = src[r * stride + off + j];
    }
}

static inline unsigned heads_copy_blocks(int64_t items) {
    int64_t b = (items + 255) / 256;
    const int64_t cap = 256 * 32;  // a few workgroups per CU, grid-stride beyond
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

hipError_t launch_heads_slice(const float* src, float* dst, int64_t rows, int64_t stride, int64_t off, int64_t width, hipStream_t st) {
    if (rows <= 0 || width <= 0) return hipSuccess;
    hipLaunchKernelGGL((heads_slice_kernel<false>), dim3(heads_copy_blocks(rows * width)), dim3(256), 0, st, src, dst, rows, stride, off, width);
    return hipGetLastError();
}

hipError_t launch_heads_unslice(const float* src, float* dst, int64_t rows, int64_t stride, int64_t off, int64_t width, hipStream_t st) {
    if (rows <= 0 || width <= 0) return hipSuccess;
    hipLaunchKernelGGL((heads_slice_kernel<true>), dim3(heads_copy_blocks(rows * width)), dim3(256), 0, st, src, dst, rows, stride, off, width);
    return hipGetLastError();
}

// A workgroup permutes 256 entries: ONE row search per entry (thread t finds where entry p0 + t comes from), then the 256 H words of the
// block are copied with consecutive threads on consecutive words of val_p. `order` (may be NULL) is applied to where the entry comes
// from: the caller's weights through an edge order, in the same copy.
__global__ __launch_bounds__(256) void permute_head_values_kernel(const int32_t* __restrict__ rowptr_p, const int32_t* __restrict__ src_begin,
                                                                  const float* __restrict__ val, float* __restrict__ val_p, int M, int nnz,
                                                                  int H, const int32_t* __restrict__ order) {
    __shared__ int s_src[256];
    const int p0 = blockIdx.x * 256, p = p0 + threadIdx.x;
    if (p < nnz) {
        const int r = row_of_entry(rowptr_p, M, p);
        const int src = src_begin[r] + (p - rowptr_p[r]);
        s_src[threadIdx.x] = order ? order[src] : src;
    }
    __syncthreads();
    const int cnt = (nnz - p0 < 256 ? nnz - p0 : 256) * H;  // words of this block (nnz H < 2^31 on this route)
    for (int i = threadIdx.x; i < cnt; i += 256) {
        const int e = i / H, h = i - e * H;
        val_p[(size_t)p0 * H + i] = val[(size_t)s_src[e] * H + h];
    }
}

hipError_t launch_permute_head_values(const int32_t* rowptr_p, const int32_t* src_begin, const float* val, float* val_p, int64_t M,
                                      int64_t nnz, int64_t H, hipStream_t st, const int32_t* order) {
    if (nnz <= 0 || H <= 0) return hipSuccess;
    if (nnz * H >= (1ll << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(permute_head_values_kernel, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, rowptr_p, src_begin, val, val_p, (int)M,
                       (int)nnz, (int)H, order);
    return hipGetLastError();
}

}  // namespace gespmm
