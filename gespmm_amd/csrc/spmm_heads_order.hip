// spmm_heads_order.hip — the multi-head product with its [nnz, H] weights read THROUGH AN EDGE ORDER (gespmm_csr_spmm_heads_order_f32 /
// _x16: the weights of CSR entry p are row order[p] of val — the backward of an attention layer on the CSC arrays, with no permuted copy
// of the weights), and the row gather behind the routes that still need such a copy (gespmm_edge_gather).
//
// The kernels are spmm_heads_kernel.h's body with ORDERED = true: the tile staging reads order[] one tile further ahead than the weights
// and gathers each entry's H words; everything after the staging is the unordered kernel's, so the bits are those of the unordered entry
// on the gathered copy. Storage order only (a plan composes the order into the copy it already makes: launch_permute_head_values), the
// 11 stateless geometries of spmm_heads.hip's table for fp32, fp16 and bf16 elements. A translation unit of its own: the kernels of
// spmm_heads.hip and spmm_heads_x16.hip stay exactly what they are.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spmm_device.h"
#include "spmm_heads.h"
#include "spmm_heads_kernel.h"

namespace gespmm {

template <int DT, int V, int S, int W>
static hipError_t launch_ordered(const HeadsArgs& a, const int32_t* order, int rpw, hipStream_t st) {
    constexpr int U = (V * S >= 8) ? 4 : 8;  // gather depth, as launch_heads (spmm_heads.hip) and launch_heads_x16
    HeadsOrderArgs args;
    int64_t nitems = 0;
    if (!heads_launch_shape<V, S, W, false>(a, rpw, static_cast<HeadsArgs*>(&args), &nitems))
        return nitems <= 0 ? hipSuccess : hipErrorInvalidConfiguration;
    args.order = order;
    hipLaunchKernelGGL((spmm_heads_kernel_t<DT, V, S, W, U, false, true>), dim3((unsigned)nitems), dim3(kThreads), 0, st, args);
    return hipGetLastError();
}

template <int DT>
static hipError_t launch_ordered_geometry(const HeadsArgs& a, const int32_t* order, const Geometry& g, hipStream_t st) {
#define GESPMM_ORDERED(V_, S_, W_) \
    if (g.vec == V_ && g.strips == S_ && g.group == W_) return launch_ordered<DT, V_, S_, W_>(a, order, g.rows_per_wave, st);
    GESPMM_ORDERED(1, 1, 4)
    GESPMM_ORDERED(1, 1, 8)
    GESPMM_ORDERED(1, 1, 16)
    GESPMM_ORDERED(1, 1, 32)
    GESPMM_ORDERED(1, 1, 64)
    GESPMM_ORDERED(4, 1, 32)
    GESPMM_ORDERED(4, 1, 64)
    GESPMM_ORDERED(4, 2, 64)
    GESPMM_ORDERED(2, 1, 64)
    GESPMM_ORDERED(2, 2, 64)
    GESPMM_ORDERED(1, 2, 64)
#undef GESPMM_ORDERED
    return hipErrorInvalidValue;
}

hipError_t launch_spmm_heads_order(const HeadsArgs& a, const int32_t* order, int dtype, const Geometry& geo, hipStream_t st) {
    if (a.tasks != nullptr || !order || a.H < 2 || a.H > kHeadsMax || a.F < 1 || a.N != a.H * a.F || a.F % geo.vec != 0)
        return hipErrorInvalidValue;
    // (a.val / a.colind / a.B may be NULL when the matrix has no entries: every load of them — and of order — sits under a position compare)
    if (!heads_geometry_served(geo, false)) return hipErrorInvalidValue;
    if (dtype == 0) return launch_ordered_geometry<0>(a, order, geo, st);
    if (dtype == kX16F16) return launch_ordered_geometry<kX16F16>(a, order, geo, st);
    if (dtype == kX16Bf16) return launch_ordered_geometry<kX16Bf16>(a, order, geo, st);
    return hipErrorInvalidValue;
}

// ----------------------------------------------------------------------------- the row gather
//
// out[i, :] = x[order[i], :] in units of U (a word, or 16 bytes where the row and both arrays allow): unit j of out is unit j % upr of
// row j / upr, so consecutive lanes write consecutive units. IT: the type the unit index is divided in (32 bits while n upr fits).
// An index outside [0, n) is never used as an address: its row of out becomes all-ones words (NaN as a float, -1 as an integer).

template <typename U, typename OT, typename IT>
__global__ __launch_bounds__(256) void edge_gather_kernel(const U* __restrict__ x, const OT* __restrict__ order, U* __restrict__ out, int64_t n,
                                                          int upr) {
    const IT total = (IT)n * (IT)upr, step = (IT)gridDim.x * 256;
    for (IT j = (IT)blockIdx.x * 256 + threadIdx.x; j < total; j += step) {
        const IT i = j / (IT)upr, u = j - i * (IT)upr;
        const int64_t src = (int64_t)order[i];
        U w;
        if (src >= 0 && src < n) {
            w = x[(uint64_t)src * (uint64_t)upr + u];
        } else {
            __builtin_memset(&w, 0xFF, sizeof w);
        }
        out[j] = w;
        if (total - j <= step) break;  // (j + step would wrap IT before it fails the compare)
    }
}

template <typename U, typename OT>
static hipError_t launch_gather_units(const void* x, const void* order, void* out, int64_t n, int upr, hipStream_t st) {
    const int64_t total = n * upr;
    int64_t b = (total + 255) / 256;
    const int64_t cap = 256 * 32;  // a few workgroups per CU, grid-stride beyond (heads_copy_blocks of spmm_heads.hip)
    const dim3 grid((unsigned)(b > cap ? cap : b));
    if (total < (1ll << 32))
        hipLaunchKernelGGL((edge_gather_kernel<U, OT, uint32_t>), grid, dim3(256), 0, st, static_cast<const U*>(x), static_cast<const OT*>(order),
                           static_cast<U*>(out), n, upr);
    else
        hipLaunchKernelGGL((edge_gather_kernel<U, OT, uint64_t>), grid, dim3(256), 0, st, static_cast<const U*>(x), static_cast<const OT*>(order),
                           static_cast<U*>(out), n, upr);
    return hipGetLastError();
}

hipError_t launch_edge_gather(const void* x, const void* order, bool order_is_64, void* out, int64_t n, int64_t row_bytes, hipStream_t st) {
    if (n <= 0 || row_bytes <= 0) return hipSuccess;
    if (row_bytes % 4 != 0 || row_bytes > (1 << 20) || !x || !order || !out) return hipErrorInvalidValue;
    const bool wide = row_bytes % 16 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    if (wide)
        return order_is_64 ? launch_gather_units<uint4, int64_t>(x, order, out, n, (int)(row_bytes / 16), st)
                           : launch_gather_units<uint4, int32_t>(x, order, out, n, (int)(row_bytes / 16), st);
    return order_is_64 ? launch_gather_units<uint32_t, int64_t>(x, order, out, n, (int)(row_bytes / 4), st)
                       : launch_gather_units<uint32_t, int32_t>(x, order, out, n, (int)(row_bytes / 4), st);
}

}  // namespace gespmm
