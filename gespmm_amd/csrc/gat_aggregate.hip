// gat_aggregate.hip — the fused GAT aggregation (gat_aggregate.h): the multi-head batch-stream kernel of spmm_heads.hip with the H
// weights of a tile entry computed from el, er and the row statistics where that kernel loads them, its launch table, and the
// elementwise kernel that materialises the same weights for the composition route. A translation unit of its own: spmm_heads_kernel
// stays exactly what it is. The kernel's body is gat_aggregate_kernel.h's at DT = 0 (fp32 B and C); gat_aggregate_x16.hip holds the
// 16-bit instantiations.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edge_dropout.h"
#include "gat_aggregate.h"
#include "gat_aggregate_kernel.h"
#include "spmm_device.h"

namespace gespmm {

// ----------------------------------------------------------------------------- the kernel (gat_aggregate_kernel.h)

template <int V, int S, int W, int U, bool TRANSPOSED>
__global__ __launch_bounds__(kThreads) void gat_aggregate_kernel(GatAggregateArgs a) {
    gat_aggregate_body<0, V, S, W, U, TRANSPOSED, false>(a, EdgeDropout{});
}

template <int V, int S, int W, int U, bool TRANSPOSED>
__global__ __launch_bounds__(kThreads) void gat_aggregate_dropout_kernel(GatAggregateArgs a, EdgeDropout drop) {
    gat_aggregate_body<0, V, S, W, U, TRANSPOSED, true>(a, drop);
}

// ----------------------------------------------------------------------------- launch table (launch_heads of spmm_heads.hip, storage order)

template <int V, int S, int W>
static hipError_t launch_gat(const GatAggregateArgs& a, int rpw, bool transposed, const EdgeDropout* drop, hipStream_t st) {
    constexpr int U = (V * S >= 8) ? 4 : 8;
    GatAggregateArgs args;
    int64_t nitems = 0;
    if (!gat_launch_shape<V, S, W>(a, rpw, &args, &nitems)) return nitems <= 0 ? hipSuccess : hipErrorInvalidConfiguration;
    if (drop) {
        if (transposed)
            hipLaunchKernelGGL((gat_aggregate_dropout_kernel<V, S, W, U, true>), dim3((unsigned)nitems), dim3(kThreads), 0, st, args, *drop);
        else
            hipLaunchKernelGGL((gat_aggregate_dropout_kernel<V, S, W, U, false>), dim3((unsigned)nitems), dim3(kThreads), 0, st, args, *drop);
        return hipGetLastError();
    }
    if (transposed) hipLaunchKernelGGL((gat_aggregate_kernel<V, S, W, U, true>), dim3((unsigned)nitems), dim3(kThreads), 0, st, args);
    else hipLaunchKernelGGL((gat_aggregate_kernel<V, S, W, U, false>), dim3((unsigned)nitems), dim3(kThreads), 0, st, args);
    return hipGetLastError();
}

hipError_t launch_gat_aggregate(const GatAggregateArgs& a, const Geometry& g, bool transposed, const EdgeDropout* drop, hipStream_t st) {
    if (drop && !drop->seed) return hipErrorInvalidValue;
    if (a.H < 1 || a.H > kHeadsMax || a.F < 1 || a.N != a.H * a.F || a.F % g.vec != 0) return hipErrorInvalidValue;
    if (!a.rowptr || !a.colind || !a.B || !a.C || !a.el || !a.er || !a.stats) return hipErrorInvalidValue;
    if (!heads_geometry_served(g, false)) return hipErrorInvalidValue;
#define GESPMM_GAT(V_, S_, W_) \
    if (g.vec == V_ && g.strips == S_ && g.group == W_) return launch_gat<V_, S_, W_>(a, g.rows_per_wave, transposed, drop, st);
    GESPMM_GAT(1, 1, 4)
    GESPMM_GAT(1, 1, 8)
    GESPMM_GAT(1, 1, 16)
    GESPMM_GAT(1, 1, 32)
    GESPMM_GAT(1, 1, 64)
    GESPMM_GAT(4, 1, 32)
    GESPMM_GAT(4, 1, 64)
    GESPMM_GAT(4, 2, 64)
    GESPMM_GAT(2, 1, 64)
    GESPMM_GAT(2, 2, 64)
    GESPMM_GAT(1, 2, 64)
#undef GESPMM_GAT
    return hipErrorInvalidValue;
}

// ----------------------------------------------------------------------------- composition route: the weights as an array, grid-stride

template <bool TRANSPOSED>
__global__ __launch_bounds__(256) void gat_weights_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ ind,
                                                          const float* __restrict__ el, const float* __restrict__ er,
                                                          const float* __restrict__ stats, float* __restrict__ w, int S, int H, int64_t n,
                                                          float slope) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int p = (int)(i / H), h = (int)(i - (int64_t)p * H);
        const int seg = row_of_entry(ptr, S, p), j = ind[p];
        const int r = TRANSPOSED ? j : seg, c = TRANSPOSED ? seg : j;
        w[i] = gat_weight(el[r * H + h], er[c * H + h], reinterpret_cast<const float2*>(stats)[r * H + h], slope);
    }
}

hipError_t launch_gat_weights(const int32_t* ptr, const int32_t* ind, const float* el, const float* er, const float* stats, float* w,
                              int64_t S, int64_t H, int64_t nnz, float slope, bool transposed, hipStream_t st) {
    if (nnz <= 0 || H <= 0) return hipSuccess;
    if (S < 1 || nnz * H >= (1ll << 31)) return hipErrorInvalidValue;
    const int64_t n = nnz * H;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;  // a few workgroups per CU, grid-stride beyond
    if (transposed)
        hipLaunchKernelGGL(gat_weights_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, ptr, ind, el, er, stats, w, (int)S, (int)H, n, slope);
    else
        hipLaunchKernelGGL(gat_weights_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, ptr, ind, el, er, stats, w, (int)S, (int)H, n, slope);
    return hipGetLastError();
}

}  // namespace gespmm
