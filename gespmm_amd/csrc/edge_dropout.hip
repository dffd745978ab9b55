// edge_dropout.hip — dropout on an [nnz, H] array of a CSR pattern with the stateless mask of edge_dropout.h: one grid-stride kernel,
// no workspace, capturable. The entry's row comes from row_of_entry, as in gat_weights_kernel (gat_aggregate.hip). y == x is allowed:
// every word is read and written by the same thread, once. TRANSPOSED: the array is in the order of (colptr, rowind) — the composition
// route of the transposed aggregation — so the segment is the column and the index the row.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edge_dropout.h"
#include "spmm_device.h"

namespace gespmm {

template <bool TRANSPOSED>
__global__ __launch_bounds__(256) void edge_dropout_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ ind,
                                                           const float* x, float* y, int S, int H, int64_t n, EdgeDropout d) {
    const uint32_t s0 = d.seed[0], s1 = d.seed[1];  // wave-uniform
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int p = (int)(i / H), h = (int)(i - (int64_t)p * H);
        const int seg = row_of_entry(ptr, S, p), j = ind[p];
        const int r = TRANSPOSED ? j : seg, c = TRANSPOSED ? seg : j;
        y[i] = edge_dropout_apply(x[i], edge_dropout_bits(s0, s1, (uint32_t)r, (uint32_t)c, (uint32_t)h), d.threshold, d.scale);
    }
}

hipError_t launch_edge_dropout(const int32_t* ptr, const int32_t* ind, const float* x, float* y, int64_t S, int64_t H, int64_t nnz,
                               const EdgeDropout& d, bool transposed, hipStream_t st) {
    if (nnz <= 0 || H <= 0) return hipSuccess;
    if (S < 1 || !d.seed || nnz * H >= (1ll << 31)) return hipErrorInvalidValue;
    const int64_t n = nnz * H;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;  // a few workgroups per CU, grid-stride beyond
    if (transposed) hipLaunchKernelGGL(edge_dropout_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, ptr, ind, x, y, (int)S, (int)H, n, d);
    else hipLaunchKernelGGL(edge_dropout_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, ptr, ind, x, y, (int)S, (int)H, n, d);
    return hipGetLastError();
}

}  // namespace gespmm
