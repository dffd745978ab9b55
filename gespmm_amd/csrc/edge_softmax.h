// edge_softmax.h — softmax over the entries of each CSR row, per head, and its backward (gespmm_edge_softmax_f32 /
// gespmm_edge_softmax_backward_f32; kernels in edge_softmax.hip).
//
// score, out, alpha, grad_alpha, grad_score are [nnz, H], row-major, in CSR edge order. For row r with entries [lo, hi) and head h:
//   forward    x_p = leaky(score[p H + h]),  m = max_p x_p,  t_p = exp(x_p - m),  out[p H + h] = t_p / sum_p t_p
//   backward   dot = sum_p alpha_p g_p,      grad[p H + h] = alpha_p (g_p - dot) (score_p >= 0 ? 1 : slope)
// leaky(x) = x >= 0 ? x : slope x; slope == 1 means none (no multiply, the backward reads no score). Empty rows write nothing.
//
// The unit of work is the (row, head) PAIR, as in sddmm_heads.h: a wavefront owns rpw consecutive rows (their rpw + 1 row pointers
// are one coalesced load, kept in a register per lane), a group of W lanes takes one pair, the 64 / W groups take consecutive pairs
// (consecutive heads of the same entries: contiguous words). Lane l of the W takes entries lo + l + t W. H is a run-time value.
//
// Summation order, fixed by the row's degree d and (M, nnz) alone — never by the head, H, capture or the run:
//   d <= L   lane l folds its entries in entry order (fmaxf for the maximum, plain adds of t_p for the sum, an fmaf chain for the dot),
//            then an xor butterfly with masks W/2 .. 1.   W = smallest power of two >= ceil(nnz / M), clamped to [4, 16].
//   d >  L   the same at W = 64 (a whole wavefront per pair): a wave-uniform branch of the one kernel — the wavefront that owns a hub row
//            walks its H pairs after its short rows. L = kLongRowThreshold.
// A row of at most kEdgeSoftmaxIT entries per lane is read once and kept in registers; a longer one is swept three times (maximum, sum,
// write; the backward twice), the later sweeps from L2. Both regimes fold in the same order, so which one ran leaves no trace.
// No atomics, no workspace, no host synchronisation: capturable. resolve_edge_softmax (select.cpp) answers W and L.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "select.h"

namespace gespmm {

// ---- the two cross-lane steps of the geometry above, shared by the kernels that use it (edge_softmax.hip, gat_backward.hip)
// Sum over the W lanes of a group: the xor butterfly W/2 .. 1, the same bits in every lane.
template <int W>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int m = W >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// Largest degree among the wavefront's 64 / W lane groups, in a scalar register.
template <int W>
__device__ __forceinline__ int wave_max_degree(int d) {
#pragma unroll
    for (int m = 32; m >= W; m >>= 1) {
        const int o = __shfl_xor(d, m, 64);
        d = o > d ? o : d;
    }
    return __builtin_amdgcn_readfirstlane(d);
}

// nnz > 0, M > 0, H >= 1, nnz H <= kSddmmMaxNnz, M <= kEdgeSoftmaxMaxRows. slope == 1: no leaky ReLU.
hipError_t launch_edge_softmax(const int32_t* rowptr, const float* score, float* out, int64_t M, int64_t H, int64_t nnz, float slope,
                               const EdgeSoftmaxLaunch& r, hipStream_t st);
// score is read only when slope != 1 (for its sign).
hipError_t launch_edge_softmax_backward(const int32_t* rowptr, const float* alpha, const float* grad_alpha, const float* score,
                                        float* grad_score, int64_t M, int64_t H, int64_t nnz, float slope, const EdgeSoftmaxLaunch& r,
                                        hipStream_t st);


// ---- the same softmax on the additive score of a graph attention layer, score[e, h] = fl(el[row(e), h] + er[colind[e], h]), which is
// never written (gespmm_gat_softmax_f32 / _backward_f32): el is [M, H], er [K, H], colind within [0, K). The score is a source trait of
// the one kernel; per pair el is loaded once, per entry colind and er (a row longer than kEdgeSoftmaxIT W entries gathers again in
// each sweep). Bits: those of the calls above on the score array the width-2 SDDMM writes. M H and K H <= kSddmmMaxNnz, K >= 1.
hipError_t launch_gat_softmax(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, float* out, int64_t M,
                              int64_t K, int64_t H, int64_t nnz, float slope, const EdgeSoftmaxLaunch& r, hipStream_t st);
// stats[r, h, :] = (m, s): the row maximum and the row sum of exp(x - m) launch_gat_softmax divides by, with ITS bits — the same lane
// geometry r, regimes, chains and hub branch, minus the pass that writes (gespmm_gat_softmax_stats_f32). Every word of [M, H, 2]
// written: empty rows (+0, +0); nnz == 0: zero-filled. One 8-byte store per pair.
hipError_t launch_gat_softmax_stats(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, float* stats, int64_t M,
                                    int64_t K, int64_t H, int64_t nnz, float slope, const EdgeSoftmaxLaunch& r, hipStream_t st);
// grad_score as launch_edge_softmax_backward, and grad_el[r, h] = the sum of the row's grad_score values as stored, every word of
// [M, H] written (empty rows +0; nnz == 0: zero-filled). colind, el, er are read only when slope != 1 (the sign of fl(el + er)).
// Summation order of grad_el, pinned: lane l adds its entries lo + l + t W in entry order, plain adds from +0, a masked position adds
// +0; then the xor butterfly W/2 .. 1 (W = 64 for d > L). The register regime and the sweep regime give the same chain.
hipError_t launch_gat_softmax_backward(const int32_t* rowptr, const int32_t* colind, const float* alpha, const float* grad_alpha,
                                       const float* el, const float* er, float* grad_score, float* grad_el, int64_t M, int64_t K, int64_t H,
                                       int64_t nnz, float slope, const EdgeSoftmaxLaunch& r, hipStream_t st);
// out[s, h] = sum over p in [ptr[s], ptr[s + 1]) of x[(order ? order[p] : p) H + h], in the order above (gespmm_edge_segment_sum_f32):
// every word of [S, H] written. r = resolve_edge_softmax(S, nnz, H). order: int32[nnz] within [0, nnz), or null. S H <= kSddmmMaxNnz.
hipError_t launch_edge_segment_sum(const int32_t* ptr, const int32_t* order, const float* x, float* out, int64_t S, int64_t H, int64_t nnz,
                                   const EdgeSoftmaxLaunch& r, hipStream_t st);

}  // namespace gespmm
