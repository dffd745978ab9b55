// edge_dropout.h — dropout on the attention coefficients of a sparsity pattern with a mask that is never stored (gespmm_edge_dropout_f32
// and the *_dropout_f32 forms of the fused GAT aggregation and backward; kernels: edge_dropout.hip, gat_aggregate.hip, gat_backward.hip).
//
// The keep / drop decision of entry (r, c) and head h is a pure function of (seed, r, c, h), stated ONCE here and callable from host and
// device code. Everything is uint32 arithmetic:
//   mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
//   bits(s0, s1, r, c, h) = mix( mix( mix(r ^ s0) ^ c ) ^ (h * 0x9E3779B9) ^ s1 )
//   keep(r, c, h) = bits >= T,   T = min(floor((double)(float)p 2^32), 2^32 - 1)           (host; a kernel argument)
//   dropout(x)    = keep ? x * s : +0,   s = 1.0f / (1.0f - p)                              (one fp32 division on the host)
// dropout is a SELECT, not a multiplication by 0: a dropped NaN / inf becomes +0. p == 0 gives T = 0 and s = 1: every entry is kept
// and x * 1 changes no bit.
//
// r and c are the row and the column of the entry IN THE PATTERN, whichever way it is walked: the walk over CSR rows sees (segment,
// index), the walk over CSC columns (index, segment), and both recompute the same decision with no CSR position and no csc_order. The
// price: two entries with the same (r, c) — a multigraph — share their decision. The two inner mixes do not depend on the head: a lane
// that owns the H heads of an entry computes them once (edge_dropout_entry), then one mix per head (edge_dropout_head).
//
// The seed is two 32-bit words of DEVICE memory, loaded wave-uniformly by every kernel with ordinary loads; nothing writes to it. No
// host synchronisation; a seed drawn on the device inside a captured region is fresh at every replay.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GESPMM_HD __host__ __device__ __forceinline__
#else
#define GESPMM_HD inline
#endif

namespace gespmm {

GESPMM_HD uint32_t edge_dropout_mix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// the part of bits() the heads of an entry share
GESPMM_HD uint32_t edge_dropout_entry(uint32_t s0, uint32_t r, uint32_t c) { return edge_dropout_mix(edge_dropout_mix(r ^ s0) ^ c); }

GESPMM_HD uint32_t edge_dropout_head(uint32_t entry, uint32_t s1, uint32_t h) { return edge_dropout_mix(entry ^ (h * 0x9E3779B9u) ^ s1); }

GESPMM_HD uint32_t edge_dropout_bits(uint32_t s0, uint32_t s1, uint32_t r, uint32_t c, uint32_t h) {
    return edge_dropout_head(edge_dropout_entry(s0, r, c), s1, h);
}

// What a kernel is given: the seed's address, the threshold and the scale of a kept entry.
struct EdgeDropout {
    const uint32_t* seed;
    uint32_t threshold;
    float scale;
};

GESPMM_HD float edge_dropout_apply(float x, uint32_t bits, uint32_t threshold, float scale) { return bits >= threshold ? x * scale : 0.0f; }

// Host side: 0 <= p < 1 (the caller has checked).
inline uint32_t edge_dropout_threshold(float p) {
    const double t = (double)p * 4294967296.0;
    return t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
}
inline EdgeDropout make_edge_dropout(float p, const void* seed) {
    return EdgeDropout{static_cast<const uint32_t*>(seed), edge_dropout_threshold(p), 1.0f / (1.0f - p)};
}

#if defined(__HIPCC__)
// y[p H + h] = dropout(x[p H + h]) for entry p in the order of (ptr, ind), S segments: (rowptr, colind), or with `transposed`
// (colptr, rowind) — the decision is that of the entry's (row, column) either way. nnz H < 2^31, S >= 1; y == x allowed.
hipError_t launch_edge_dropout(const int32_t* ptr, const int32_t* ind, const float* x, float* y, int64_t S, int64_t H, int64_t nnz,
                               const EdgeDropout& d, bool transposed, hipStream_t st);
#endif

}  // namespace gespmm
