// gatv2_score.h — the GATv2 edge score and its gradients (gespmm_gatv2_score_f32, gespmm_gatv2_score_backward_f32; kernels:
// gatv2_score.hip). fp32, CSR form only; no plan, no composition route, no environment pin.
//
// xl is [M, H, F] (the aggregating node: the row of an entry), xr is [K, H, F] (the neighbour: the column), att is [H, F], score is
// [nnz, H] in CSR entry order, head-minor — what the edge softmax reads:
//   score[p H + h] = sum_f att[h, f] * leaky(fl(xl[row(p), h, f] + xr[col(p), h, f]))        leaky(t) = t >= 0 ? t : slope * t
// t is ONE fp32 add; slope == 1 means no multiply. The non-linearity sits inside the sum, so nothing here splits into a row term plus
// a column term, and nothing of size nnz H F exists in either direction.
//
// FORWARD. The geometry is that of sddmm_heads_kernel (sddmm_heads.h, CSR form), restated in gatv2_score.hip: the unit of work is the
// (entry, head) pair q = p H + h; a wavefront owns epw consecutive entries — epw H consecutive words of score — and resolves their row
// and column ONCE for all H heads (one wavefront-wide row search, the row-pointer window in LDS); a group of W lanes covers a head
// slice with V floats per load, and the slice of att for head h is a third operand at the same vector positions. (V, W, epw) come from
// resolve_gatv2_score (select.cpp) at WIDTH F for the THREE operand addresses: V divides F and 4 V bytes divide all three bases, so no
// vector spans two heads.
// Pinned order: lane l of W runs ONE chain
//   acc = fmaf(att[h, j], leaky(fl(xl_j + xr_j)), acc)     from +0, over j = l V + i + t W V, i ascending inside a vector, t ascending,
// then the xor butterfly with masks W/2 .. 1; lane 0 stores. A lane past the slice contributes fmaf(0, 0, 0) (which leaves acc as it is).
//
// BACKWARD. One kernel serves both node terms. For segment s with entries p in [ptr[s], ptr[s + 1]), c = ind[p], q = order ? order[p]
// : p and t = fl(x_seg[s, h, f] + x_ind[c, h, f]):
//   m_pf              = t >= 0 ? att[h, f] : fl(att[h, f] * slope)              (att[h, f] for every t when slope == 1)
//   grad_x[s, h, f]   = chain over p ascending from +0 of fmaf(grad_score[q H + h], m_pf, acc)
//   att_part[s, h, f] = chain over p ascending from +0 of fmaf(grad_score[q H + h], leaky(t), acc)         (only when att_part != NULL)
// Row pass: (rowptr, colind, no order, x_seg = xl, x_ind = xr) gives grad_xl and att_part. Column pass: (colptr, rowind, csc_order,
// x_seg = xr, x_ind = xl, no att_part) gives grad_xr. fp32 addition commutes bit for bit, so both passes see the same t and the leaky
// factor is the same in both without being stored. grad_att is att_part summed over its first axis by the caller.
// Pinned order: ONE fp32 fmaf chain per output word, in segment order — the contract of the multi-head product (spmm_heads.h). Lane
// geometry, vector width and unroll depth leave no trace in the bits; consequently there is no long-row pass: a hub segment is walked
// by one lane group (a limit). Geometry: the row walk of the streaming product at width N = H F — a group of W lanes per segment, lanes
// contiguous in (h, f), V = 4 (16-byte vectors) when F % 4 == 0 and every dense operand is 16-byte aligned, else V = 1; the group loads
// W indices at a time, coalesced, and broadcasts them; four gathers of x_ind rows are in flight per lane; strips of W V words when N
// exceeds the group's span. Every word of grad_x (and of att_part) is written; an empty segment writes +0.
//
// Safety rules: every load is clamped to a valid word and dropped by a select, trip counts are wave-uniform, only stores
// are predicated, a wavefront past the end returns whole. No atomics, no workspace, no allocation, no host synchronisation: both
// launches are capturable.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "select.h"

namespace gespmm {

// nnz >= 1, M, K, H, F >= 1; nnz H, M H F and K H F <= kSddmmMaxNnz (32-bit word positions); colind within [0, K). r =
// resolve_gatv2_score(...) for the addresses of xl, xr and att.
hipError_t launch_gatv2_score(const int32_t* rowptr, const int32_t* colind, const float* xl, const float* xr, const float* att,
                              float* score, int64_t M, int64_t nnz, int64_t H, int64_t F, float slope, const Gatv2ScoreLaunch& r,
                              hipStream_t st);

// S, T, H, F, nnz >= 1; nnz H, S H F and T H F <= kSddmmMaxNnz; ind within [0, T), order (when given) within [0, nnz). att_part may be
// null. vec4: F % 4 == 0 and x_seg, x_ind, att, grad_x and att_part are 16-byte aligned.
hipError_t launch_gatv2_score_backward(const int32_t* ptr, const int32_t* ind, const int32_t* order, const float* grad_score,
                                       const float* x_seg, const float* x_ind, const float* att, float* grad_x, float* att_part, int64_t S,
                                       int64_t H, int64_t F, int64_t nnz, float slope, bool vec4, hipStream_t st);

}  // namespace gespmm
