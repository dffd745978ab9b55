// gat_backward.h — the fused backward of a graph attention layer for its two per-node score terms (gespmm_gat_backward_el_f32 /
// gespmm_gat_backward_er_f32; kernel in gat_backward.hip): grad_el and grad_er with no [nnz, H] array.
//
// el, grad_el, delta are [M, H]; er, grad_er [K, H]; stats [M, H, 2] (launch_gat_softmax_stats); grad_out [M, H, F]; feat [K, H, F].
// For entry p of row r with column c = colind[p], and head h:
//   w_p        = weight(r, c, h)                          gat_weight (gat_aggregate.h): the bits of alpha
//   g_p        = sum_f grad_out[r, h, f] feat[c, h, f]
//   delta[r,h] = sum_{p in row r} w_p g_p
//   gs_p       = w_p (g_p - delta[r, h]) (fl(el[r, h] + er[c, h]) >= 0 ? 1 : slope)          (the factor only when slope != 1)
//   grad_el[r, h] = sum_{p in row r} gs_p                 grad_er[c, h] = sum_{p in column c} gs_p
// gs_p is never stored: it is a function of node-sized words alone, so the pass over the rows (launch_gat_backward_el: rowptr, colind;
// writes delta and grad_el) and the pass over the columns (launch_gat_backward_er: colptr, rowind; reads delta, writes grad_er; no
// csc_order) each compute it, with the same bits.
//
// Lane geometry: edge_softmax.h's. The unit of work is the (segment, head) pair — segments are the M rows in the first pass, the K
// columns in the second; a wavefront owns rpw consecutive segments (one coalesced load of their pointers), a group of W lanes takes
// one pair, the 64 / W groups consecutive pairs, lane l entries lo + l + t W; segments of more than L entries take a whole wavefront
// per pair (W = 64) in a wave-uniform branch of the same kernel. W, L, rpw = resolve_edge_softmax(segments, nnz, H).
//
// Pinned orders — fixed by the segment's degree and (segments, nnz) alone, never by the head, H, F's divisors, alignment or capture:
//   g_p      ONE lane computes the whole dot: acc = fmaf(a_f, b_f, acc) over ascending f from +0. The loads are 16 bytes wide when
//            F % 4 == 0 and both operands sit on 16-byte boundaries, 4 bytes wide otherwise; the chain is the same.
//   delta    the `dot` of the edge softmax's backward: per lane dot = fmaf(w_p, g_p, dot) in entry order from +0, a masked position
//            leaves it unchanged; then the xor butterfly W/2 .. 1.
//   gs_p     r = w * (g - delta); if (slope != 1) r *= factor;      two (three) roundings, in this order.
//   grad_el, grad_er   per lane s += gs_p in entry order from +0, a masked position adds +0; then the butterfly — the chain of
//            launch_gat_softmax_backward's grad_el and of launch_edge_segment_sum.
// Hence, where g_p itself has the bits of the multi-head SDDMM (always when its partial sums are exact), delta, grad_el and grad_er
// have the bits of launch_gat_softmax, launch_sddmm_heads, launch_gat_softmax_backward and launch_edge_segment_sum(colptr, .., order).
//
// A segment of at most kEdgeSoftmaxIT entries per lane keeps w and g in registers (one gather of the F-wide rows gives delta AND
// grad_el); a longer row is swept twice in the first pass, the second sweep computing w and g again. The second pass is one sweep in
// both regimes: delta is an input. Both regimes fold in the same order. No atomics, no workspace, no host synchronisation: capturable.
// Every word of delta, grad_el and grad_er is written (empty segments +0; nnz == 0: zero-filled, nothing launched).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "select.h"

namespace gespmm {

struct EdgeDropout;  // edge_dropout.h

// An element of grad_out / feat as the kernels address it: a float, or the 16 bits of an fp16 / bf16 value.
template <int DT>
struct GatBackwardElem {
    using type = uint16_t;
};
template <>
struct GatBackwardElem<0> {
    using type = float;
};
template <int DT>
using gb_elem_t = typename GatBackwardElem<DT>::type;

// drop != nullptr (gespmm_gat_backward_{el,er}_dropout_f32): g_p is replaced by g'_p = dropout(g_p) — edge_dropout.h's mask of (r, c, h),
// one rounding fl(g_p s) or +0 — directly after its chain; delta, gs_p and the sums are the statements above on g'_p, w_p the undropped
// weight. The bits are then those of the composition with launch_edge_dropout between the SDDMM and the softmax's backward.
//
// M, K >= 1, H, F >= 1; nnz H, M H, K H, M H F and K H F <= kSddmmMaxNnz (32-bit word positions). r = resolve_edge_softmax(M, nnz, H).
hipError_t launch_gat_backward_el(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, const float* stats,
                                  const float* grad_out, const float* feat, float* delta, float* grad_el, int64_t M, int64_t K, int64_t H,
                                  int64_t F, int64_t nnz, float slope, const EdgeSoftmaxLaunch& r, const EdgeDropout* drop, hipStream_t st);
// ... r = resolve_edge_softmax(K, nnz, H).
hipError_t launch_gat_backward_er(const int32_t* colptr, const int32_t* rowind, const float* el, const float* er, const float* stats,
                                  const float* delta, const float* grad_out, const float* feat, float* grad_er, int64_t M, int64_t K,
                                  int64_t H, int64_t F, int64_t nnz, float slope, const EdgeSoftmaxLaunch& r, const EdgeDropout* drop,
                                  hipStream_t st);

// ---- The GROUP form (kernels in gat_backward_group.hip): the same two passes, the same segment geometry, regimes and pinned orders of
// delta, gs_p, grad_el and grad_er — only g_p is computed differently. The 64 lanes of a wavefront also form 64 / W_d dot sub-groups of
// W_d contiguous lanes, (4, W_d) = resolve_sddmm's answer at WIDTH F for 16-byte aligned operands (W_d the smallest power of two in
// 4 .. 64 with 8 W_d >= F, independent of the segment width W); per batch of entries a sub-group serves, in W_d steps, the entry each
// of its lanes owns, and
//   g_p      lane q of the W_d runs ONE chain acc = fmaf(a_j, b_j, acc) from +0 over j = 4 q + i + 4 W_d t (i ascending in a vector,
//            t < 2 ascending; a lane past the slice keeps +0), then the xor butterfly W_d / 2 .. 1
// which is launch_sddmm_heads' order at (4, W_d), in every form of that kernel, H = 1 included. Hence on ANY operands:
//   grad_el and grad_er have the bits of launch_gat_softmax, launch_sddmm_heads, launch_gat_softmax_backward and
//   launch_edge_segment_sum(colptr, .., order); delta has them in the pairs whose products alpha * grad_alpha are exact (the fmaf chain
//   rounds once where the composition rounds twice: the lane form's caveat, unchanged); with drop != nullptr they are the bits of that
//   composition with launch_edge_dropout between the SDDMM and the softmax's backward.
// Form rule (resolve_gat_backward, select.cpp — the one place): the group form is ELIGIBLE when F % 4 == 0, 16 <= F <= 512 and grad_out
// and feat are both 16-byte aligned (V is then always 4: the bits depend on F alone); an eligible launch takes it where F >=
// kGatBackwardGroupMinF (measured; 0: nowhere) or the pin GESPMM_GAT_BACKWARD_FORM=group says so; =lane pins the lane form. Every other
// launch takes the lane form, whose contract above stands. r.form == kGatBackwardGroup; a launch outside the rule is refused
// (hipErrorInvalidValue). nnz >= 1 (the lane form's entry serves nnz == 0). No atomics, no LDS, no workspace: capturable.
hipError_t launch_gat_backward_group_el(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, const float* stats,
                                        const float* grad_out, const float* feat, float* delta, float* grad_el, int64_t M, int64_t K,
                                        int64_t H, int64_t F, int64_t nnz, float slope, const GatBackwardLaunch& r, const EdgeDropout* drop,
                                        hipStream_t st);
hipError_t launch_gat_backward_group_er(const int32_t* colptr, const int32_t* rowind, const float* el, const float* er, const float* stats,
                                        const float* delta, const float* grad_out, const float* feat, float* grad_er, int64_t M, int64_t K,
                                        int64_t H, int64_t F, int64_t nnz, float slope, const GatBackwardLaunch& r, const EdgeDropout* drop,
                                        hipStream_t st);

// ---- fp16 / bf16 grad_out and feat (gespmm_gat_backward_{el,er}_x16; kernels in gat_backward_x16.hip and gat_backward_group_x16.hip: the
// two bodies above as templates on the element type). dtype kX16F16 / kX16Bf16, one type per call; el, er, stats, delta, grad_el and
// grad_er stay fp32, as do the weights, the dropout arithmetic and every chain. Each 16-bit element is widened, exactly, at its fmaf and
// no 16-bit word is written: nothing is rounded that the fp32 kernels do not round. r = resolve_gat_backward_x16 (select.h).
//   lane form   the contract at the top of this file; a load brings r.V ELEMENTS, 8 / 4 / 2 / 1 (F % V == 0, 2 V bytes divide both
//               addresses — refused otherwise). The chain does not see V: delta, grad_el and grad_er have the bits of
//               launch_gat_backward_el / _er on the widened operands, whatever either side's load width.
//   group form  the contract above at V = 4 ELEMENTS per lane and step (one 8-byte load): W_d, lane positions and butterfly are those of
//               the fp32 group form at width F, so the results have the bits of launch_gat_backward_group_el / _er on the widened
//               operands. Eligible when F % 4 == 0, 16 <= F <= 512 and both operands are 8-byte aligned.
// Sizes, nnz == 0, safety rules, capture: as the fp32 entries. No LDS, no atomics, no workspace.
hipError_t launch_gat_backward_el_x16(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, const float* stats,
                                      const void* grad_out, const void* feat, int dtype, float* delta, float* grad_el, int64_t M, int64_t K,
                                      int64_t H, int64_t F, int64_t nnz, float slope, const GatBackwardLaunch& r, const EdgeDropout* drop,
                                      hipStream_t st);
hipError_t launch_gat_backward_er_x16(const int32_t* colptr, const int32_t* rowind, const float* el, const float* er, const float* stats,
                                      const float* delta, const void* grad_out, const void* feat, int dtype, float* grad_er, int64_t M,
                                      int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, const GatBackwardLaunch& r,
                                      const EdgeDropout* drop, hipStream_t st);
hipError_t launch_gat_backward_group_el_x16(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, const float* stats,
                                            const void* grad_out, const void* feat, int dtype, float* delta, float* grad_el, int64_t M,
                                            int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, const GatBackwardLaunch& r,
                                            const EdgeDropout* drop, hipStream_t st);
hipError_t launch_gat_backward_group_er_x16(const int32_t* colptr, const int32_t* rowind, const float* el, const float* er, const float* stats,
                                            const float* delta, const void* grad_out, const void* feat, int dtype, float* grad_er, int64_t M,
                                            int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, const GatBackwardLaunch& r,
                                            const EdgeDropout* drop, hipStream_t st);

}  // namespace gespmm
