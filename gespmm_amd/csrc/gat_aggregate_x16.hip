// gat_aggregate_x16.hip — the fused GAT aggregation on 16-bit features (gespmm_gat_aggregate_x16 / _dropout_x16: IEEE fp16 / bfloat16 B
// and C; el, er, stats and the weights fp32; fp32 sums rounded once at the store): the kernel body of gat_aggregate_kernel.h instantiated
// on the two 16-bit element types, and its launch table. A translation unit of its own: the fp32 kernels of gat_aggregate.hip stay
// exactly what they are.
//
// The kernels work in 32-bit words, so a geometry here is the one select.cpp resolves for the width in WORDS, H F / 2, with V words per
// lane and strip and V | F / 2 (a lane's vector stays inside one head): the 11 geometries of launch_gat_aggregate, for fp16 and bf16,
// forward and transposed, plain and with dropout — 88 kernels.
//
// Gathers in flight (U): the fp32 rule, V S >= 8 ? 4 : 8, counts words — and a word now feeds two accumulators, so a lane holds 2 V S
// sums next to U V S gathered words, the tile state (an index two tiles ahead, 4 kHeadsMax words of terms one tile ahead) and, with
// dropout, the seed and the entry's mask word. Compiled for gfx950, every one of the 88 instantiations stays out of scratch at the fp32
// U — the widest, bf16 (V, S, W) = (4, 2, 64) with dropout, 16 sums + 32 gathered words, takes 167 VGPRs — so no geometry lowers it
// (DESIGN 3.30 has the table). The build fails if any instantiation spills or has a private segment (Makefile).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gat_aggregate_kernel.h"

namespace gespmm {

template <int DT, int V, int S, int W, int U, bool TRANSPOSED>
__global__ __launch_bounds__(kThreads) void gat_aggregate_x16_kernel(GatAggregateArgs a) {
    gat_aggregate_body<DT, V, S, W, U, TRANSPOSED, false>(a, EdgeDropout{});
}

template <int DT, int V, int S, int W, int U, bool TRANSPOSED>
__global__ __launch_bounds__(kThreads) void gat_aggregate_dropout_x16_kernel(GatAggregateArgs a, EdgeDropout drop) {
    gat_aggregate_body<DT, V, S, W, U, TRANSPOSED, true>(a, drop);
}

template <int DT, int V, int S, int W>
static hipError_t launch_gat_x16(const GatAggregateArgs& a, int rpw, bool transposed, const EdgeDropout* drop, hipStream_t st) {
    constexpr int U = (V * S >= 8) ? 4 : 8;  // gather depth in words: the fp32 rule (above)
    GatAggregateArgs args;
    int64_t nitems = 0;
    if (!gat_launch_shape<V, S, W>(a, rpw, &args, &nitems)) return nitems <= 0 ? hipSuccess : hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)nitems), block(kThreads);
    if (drop) {
        if (transposed) hipLaunchKernelGGL((gat_aggregate_dropout_x16_kernel<DT, V, S, W, U, true>), grid, block, 0, st, args, *drop);
        else hipLaunchKernelGGL((gat_aggregate_dropout_x16_kernel<DT, V, S, W, U, false>), grid, block, 0, st, args, *drop);
        return hipGetLastError();
    }
    if (transposed) hipLaunchKernelGGL((gat_aggregate_x16_kernel<DT, V, S, W, U, true>), grid, block, 0, st, args);
    else hipLaunchKernelGGL((gat_aggregate_x16_kernel<DT, V, S, W, U, false>), grid, block, 0, st, args);
    return hipGetLastError();
}

template <int DT>
static hipError_t launch_gat_x16_geometry(const GatAggregateArgs& a, const Geometry& g, bool transposed, const EdgeDropout* drop, hipStream_t st) {
#define GESPMM_GAT_X16(V_, S_, W_) \
    if (g.vec == V_ && g.strips == S_ && g.group == W_) return launch_gat_x16<DT, V_, S_, W_>(a, g.rows_per_wave, transposed, drop, st);
    GESPMM_GAT_X16(1, 1, 4)
    GESPMM_GAT_X16(1, 1, 8)
    GESPMM_GAT_X16(1, 1, 16)
    GESPMM_GAT_X16(1, 1, 32)
    GESPMM_GAT_X16(1, 1, 64)
    GESPMM_GAT_X16(4, 1, 32)
    GESPMM_GAT_X16(4, 1, 64)
    GESPMM_GAT_X16(4, 2, 64)
    GESPMM_GAT_X16(2, 1, 64)
    GESPMM_GAT_X16(2, 2, 64)
    GESPMM_GAT_X16(1, 2, 64)
#undef GESPMM_GAT_X16
    return hipErrorInvalidValue;
}

// `a` is the launch in WORDS: a.B / a.C the 16-bit arrays, a.N = H F / 2, a.F = F / 2 (gat_aggregate.h).
hipError_t launch_gat_aggregate_x16(const GatAggregateArgs& a, int dtype, const Geometry& g, bool transposed, const EdgeDropout* drop,
                                    hipStream_t st) {
    if (drop && !drop->seed) return hipErrorInvalidValue;
    if (a.H < 1 || a.H > kHeadsMax || a.F < 1 || a.N != a.H * a.F || a.F % g.vec != 0) return hipErrorInvalidValue;
    if (!a.rowptr || !a.colind || !a.B || !a.C || !a.el || !a.er || !a.stats) return hipErrorInvalidValue;
    if (!heads_geometry_served(g, false)) return hipErrorInvalidValue;
    if (dtype == kX16F16) return launch_gat_x16_geometry<kX16F16>(a, g, transposed, drop, st);
    if (dtype == kX16Bf16) return launch_gat_x16_geometry<kX16Bf16>(a, g, transposed, drop, st);
    return hipErrorInvalidValue;
}

}  // namespace gespmm
