// gat_aggregate.h — internal interface of the fused GAT aggregation (gespmm_gat_aggregate_f32; kernels: gat_aggregate.hip).
//
// The multi-head product of spmm_heads.h with the weights COMPUTED, not loaded: no [nnz, H] array exists. For entry p of segment i,
// j = ind[p], and head h
//   forward     (ptr, ind) = (rowptr, colind)   w = weight(i, j, h)       C[i, h F + f] = fmaf(w, B[j, h F + f], acc)
//   transposed  (ptr, ind) = (colptr, rowind)   w = weight(j, i, h)       the same chain
//   weight(r, c, h) = __expf(leaky(fl(el[r H + h] + er[c H + h])) - stats[r, h, 0]) / stats[r, h, 1]
// — the expression of softmax_pair (edge_softmax.hip) on the (m, s) launch_gat_softmax_stats stored, hence the bits of the alpha array
// launch_gat_softmax writes; the chain is launch_spmm_heads's: ascending entries from +0, one fp32 chain per output element. el is
// [M, H], er [K, H], stats [M, H, 2] in both modes; the segments are the M rows (forward) or the K columns (transposed).
// leaky(x) = x >= 0 ? x : slope x at every slope: slope == 1 multiplies by one, which changes no bit.
#pragma once
#include "spmm_heads.h"

namespace gespmm {

// The ONE expression of a weight, shared by the aggregation kernel, the composition and the fused backward (gat_backward.hip):
// softmax_pair's, term for term.
__device__ __forceinline__ float gat_weight(float el, float er, float2 ms, float slope) {
    float x = el + er;
    x = x >= 0.0f ? x : slope * x;
    return __expf(x - ms.x) / ms.y;
}

// rowptr / colind = (ptr, ind), M = segments, N = H F, val unused. 1 <= H <= kHeadsMax (H = 1 runs the kernel too).
struct GatAggregateArgs : SpmmArgs {
    int32_t H;
    int32_t F;
    const float* el;
    const float* er;
    const float* stats;
    float slope;
};

// What a weight is computed from, as the entry point receives it.
struct GatTerms {
    const float* el;
    const float* er;
    const float* stats;
    float slope;
};

struct EdgeDropout;  // edge_dropout.h

// One kernel: the geometries heads_geometry_served serves without a plan, 32-bit offsets. hipErrorInvalidValue otherwise.
// drop != nullptr: the staged weight is dropout(weight(r, c, h)) with edge_dropout.h's mask — the same (r, c) in both modes.
hipError_t launch_gat_aggregate(const GatAggregateArgs& a, const Geometry& geo, bool transposed, const EdgeDropout* drop, hipStream_t st);
// The composition's first step: w[p H + h] = weight(..) of entry p in the order of (ptr, ind), S segments. nnz H < 2^31.
hipError_t launch_gat_weights(const int32_t* ptr, const int32_t* ind, const float* el, const float* er, const float* stats, float* w,
                              int64_t S, int64_t H, int64_t nnz, float slope, bool transposed, hipStream_t st);

}  // namespace gespmm
