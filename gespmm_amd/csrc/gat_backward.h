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

}  // namespace gespmm
