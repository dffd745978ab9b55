// gatv2_score.h — the GATv2 edge score and its gradients (gespmm_gatv2_score_f32, gespmm_gatv2_score_backward_f32; kernels:
// gatv2_score.hip). fp32, CSR form only; no plan, no composition route, no environment pin. The form on fp16 / bf16 node operands
// (gespmm_gatv2_score_x16, gespmm_gatv2_score_backward_x16; kernels: gatv2_score_x16.hip) is described at the end of this header.
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

// ---- the same two on 16-bit node operands (gespmm_gatv2_score_x16, gespmm_gatv2_score_backward_x16; kernels: gatv2_score_x16.hip).
// xl, xr, x_seg, x_ind and grad_x are fp16 or bf16 (dtype kX16F16 / kX16Bf16, one type per call); att, grad_score, score and att_part
// stay fp32 — att is a parameter of H F words whose gradient is a sum over nodes, and everything edge-sized is fp32 in this library.
// The arithmetic is the fp32 contract above, unchanged: every 16-bit element is widened exactly at its use (widen_x16, spmm_device.h;
// subnormals included), t = fl32(widen(xl_j) + widen(xr_j)) is ONE fp32 add, the branch is t >= 0, the forward is the pinned lane chain
// and butterfly, the backward one fmaf chain per output word in segment order with m = t >= 0 ? att : fl(att slope). grad_x is rounded
// ONCE, at the store (narrow_x16: to nearest even, overflow to +-inf, NaN stays NaN). No packed-fp16 arithmetic and no dot2.
// Consequences: on equal (V, W) the forward has the bits of the fp32 kernel on the widened operands; the backward's att_part has the
// bits of the fp32 kernel on the widened operands whatever the geometry, and grad_x is that kernel's grad_x rounded once.
//
// FORWARD geometry: the fp32 kernel's with a lane's vector counted in ELEMENTS, V in {8, 4, 2, 1} — a dwordx4 / dwordx2 / dword / ushort
// load of xl and xr, and att's V floats at the same element positions (two dwordx4 loads at V = 8). V is the largest value that divides
// F, whose 2 V bytes divide the addresses of xl and xr, and whose min(4 V, 16) bytes divide the address of att; W and epw are the
// existing resolvers' at element size 2 for width F (resolve_gatv2_score_x16, select.cpp). The bits depend on (V, W) alone. Pairs in
// flight per lane group: 4 up to V = 4, 2 at V = 8 (registers: gatv2_score_x16.hip).
// BACKWARD geometry: the fp32 row walk at width N = H F with V elements per lane, four gathers in flight: V the largest of 8 / 4 / 2 / 1
// that divides F (no vector spans two heads), whose 2 V bytes divide the addresses of x_seg, x_ind and grad_x and whose min(4 V, 16)
// bytes divide those of att and att_part (gatv2_score_x16_vec) — 16-byte vectors when F % 8 == 0 and every dense operand is 16-byte
// aligned; V = 1 serves any F and any 2-byte aligned address. Geometry leaves no trace in the bits.
// The safety rules and the limits are those above (positions count 16-bit ELEMENTS); no long-segment pass.

// nnz >= 1, M, K, H, F >= 1; nnz H, M H F and K H F <= kSddmmMaxNnz; colind within [0, K). r = resolve_gatv2_score_x16(...) for the
// addresses of xl, xr and att.
hipError_t launch_gatv2_score_x16(const int32_t* rowptr, const int32_t* colind, const void* xl, const void* xr, const float* att,
                                  float* score, int dtype, int64_t M, int64_t nnz, int64_t H, int64_t F, float slope,
                                  const Gatv2ScoreLaunch& r, hipStream_t st);

// The backward's vector: x_align the least alignment (bytes, a power of two <= 16) of the 16-bit operands, f_align that of the fp32 ones.
int gatv2_score_x16_vec(int64_t F, int x_align, int f_align);

// S, T, H, F, nnz >= 1; limits as above. att_part may be null. V = gatv2_score_x16_vec(F, ...) for x_seg, x_ind, grad_x | att, att_part.
hipError_t launch_gatv2_score_backward_x16(const int32_t* ptr, const int32_t* ind, const int32_t* order, const float* grad_score,
                                           const void* x_seg, const void* x_ind, const float* att, void* grad_x, float* att_part, int dtype,
                                           int64_t S, int64_t H, int64_t F, int64_t nnz, float slope, int V, hipStream_t st);

}  // namespace gespmm
