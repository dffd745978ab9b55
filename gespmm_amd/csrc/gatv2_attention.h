// gatv2_attention.h — fused GATv2 attention over the entries of a sparsity pattern: score, softmax and aggregation in one sweep, and its
// backward (gespmm_gatv2_attention_f32, gespmm_gatv2_attention_backward_row_f32, gespmm_gatv2_attention_backward_col_f32 and their
// *_dropout_f32 forms; kernels: gatv2_attention.hip). fp32, no plan, no composition route, no environment pin.
//
// xl is [M, H, F] (the aggregating node: the row of an entry), xr is [K, H, F] (the neighbour: the column), att is [H, F]; out and
// grad_out are [M, H, F], stats is [M, H, 2], delta is [M, H]. slope == 1 means no multiply. For entry p of row r with column c and head h:
//   t_pf       = fl(xl[r, h, f] + xr[c, h, f])                 ONE fp32 add, as in gatv2_score.h
//   s_p        = sum_f att[h, f] * leaky(t_pf)                 leaky(t) = t >= 0 ? t : fl(slope * t)
//   a_p        = exp(s_p - m) / l            m = max_p s_p,  l = sum_p exp(s_p - m)            stats[r, h] = (m, l)
//   out[r,h,:] = sum_p a_p xr[c, h, :]
// The neighbour's slice is both the score's operand and the aggregated value: ONE gathered row per entry serves the whole forward.
// Nothing of size nnz is read, written or allocated apart from the index arrays, in either direction.
//
// GEOMETRY, all three kernels: that of dot_attention.h. The unit of work is the (segment, head) pair: segments are the rows in the forward
// and the row pass, the columns in the column pass. A group of W lanes owns a pair; the 64 / W groups of a wavefront take consecutive
// pairs; a wavefront past the end returns whole. The lanes of a group are contiguous in f, V floats per load, 8 floats per lane and
// operand: (V, W) = resolve_gatv2_attention(F, alignment) — resolve_sddmm's rule at WIDTH F for the least aligned of xl, xr, att and the
// dense results, the rule resolve_gatv2_score and resolve_dot_attention share: V the widest of 4 / 2 / 1 that divides F and whose bytes
// divide every dense operand's address (no vector spans two heads), W the smallest power of two in 4 .. 64 with 8 W >= F. F > 512 is NOT
// SERVED (kGatv2AttentionMaxF): the entry points answer GESPMM_ERR_UNSUPPORTED and launch nothing. The segment's own slices (xl or xr,
// att, and grad_out in the row pass) and all accumulators live in registers for the whole segment. The group reads W indices at a
// time, coalesced, and broadcasts them. A hub segment is walked by its one lane group (a limit, as in gatv2_score.h and dot_attention.h).
//
// GATHERS IN FLIGHT. The forward and the row pass gather ONE row per entry (xr[c, h, :]) and request the rows of FOUR entries before the
// first is used; the column pass gathers two rows and three words per entry (xl, grad_out, stats, delta) and requests those of TWO
// entries. The fused dot attention was found latency-bound with two entries — four gathered rows — in flight per lane group (DESIGN
// section 10 item 9); four rows in the same registers is the depth here. That depth is CHOSEN BY THAT REASONING, NOT MEASURED.
//
// PINNED ORDERS.
//   s_p: lane l runs ONE chain acc = fmaf(att_j, leaky(fl(xl_j + xr_j)), acc) from +0 over j = l V + i + t W V (i ascending inside a vector,
//   t ascending below ceil(F / (W V))), then the xor butterfly W/2 .. 1: the order of gatv2_score.h, so on equally aligned operands s_p
//   has the BITS of gespmm_gatv2_score_f32. A lane past the slice contributes fmaf(0, 0, acc).
//   dot(x, y): the pinned dot of dot_attention.h (the same lane positions with fmaf(x_j, y_j, acc)).
//   The fp32 add and fmaf(a, b, acc) commute in their two factors, so the row pass and the column pass compute THE SAME BITS of t, s_p
//   and g_p. Every per-word accumulation is one chain per output word in segment (entry) order. The head, H, alignment, capture and
//   run leave no trace beyond V (which moves the lane positions of s_p and the dots).
//
// FORWARD (rowptr, colind -> out, stats). One sweep over the row with the online softmax of dot_attention.h; per entry, in entry order:
//   m' = fmaxf(m, s_p);  c = __expf(m - m');  t = __expf(s_p - m');  l = fmaf(l, c, t);  acc_f = fmaf(t, xr_f, fl(acc_f * c));  m = m'
// The first entry starts from m = s_p, l = 0, acc = 0, which gives m = s_p, l = 1, acc = xr with no exp(-inf - ..) (__expf(0) == 1).
// out = acc / l; (m, l) is one 8-byte store per pair. Every word of out and stats is written: an empty row writes +0 everywhere.
//
// BACKWARD, ROW PASS (rowptr, colind; reads xl, xr, att, stats, out, grad_out; writes delta, grad_xl, att_part):
//   delta[r, h]       = dot(grad_out[r, h, :], out[r, h, :])
//   a_p = __expf(s_p - m) / l        g_p = dot(grad_out[r, h, :], xr[c, h, :])        ds_p = a_p * (g_p - delta)
//   m_pf              = t_pf >= 0 ? att[h, f] : fl(att[h, f] * slope)
//   grad_xl[r, h, f]  = chain over p of fmaf(ds_p, m_pf, acc)
//   att_part[r, h, f] = chain over p of fmaf(ds_p, leaky(t_pf), acc)          (only when att_part != NULL; grad_att is its sum over r)
// BACKWARD, COLUMN PASS (colptr, rowind — no csc_order; reads xl, xr, att, stats, delta, grad_out; writes grad_xr). Column c's xr slice
// and att are held; per entry with row r the pass gathers xl[r, h, :], grad_out[r, h, :], stats[r, h] and delta[r, h]; t, s_p, a_p, g_p
// and ds_p have the bits of the row pass. Two chains per word, added ONCE at the store:
//   grad_xr[c, h, f]  = fl( chain_p fmaf(ds_p, m_pf, acc1)  +  chain_p fmaf(a_p, grad_out[r, h, f], acc2) )
//
// DROPOUT on the coefficients (drop != nullptr; edge_dropout.h: keep is a function of (seed, r, c, h), so the entries of a multigraph
// with the same (row, column) share it), placed where dot_attention.h places it. Forward: l sums every entry, acc takes
// fl(t * keep_scale) for a kept entry and +0 for a dropped one. Backward: g_p becomes g'_p = fl(g_p * keep_scale) or +0 directly after
// its chain, delta stays dot(grad_out, out), the second chain of grad_xr uses fl(a_p * keep_scale) or +0.
//
// Safety rules: every load is clamped to a valid word and dropped by a select, trip counts are wave-uniform, only stores
// are predicated, a wavefront past the end returns whole. No atomics, no workspace, no allocation, no host synchronisation: all
// launches are capturable. Plain C++ / HIP, no inline assembly.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edge_dropout.h"
#include "select.h"

namespace gespmm {

// M, K, H, F, nnz >= 1; F <= kGatv2AttentionMaxF; nnz, M H F, K H F and 2 M H <= kSddmmMaxNnz (32-bit word positions); colind within
// [0, K); r = resolve_gatv2_attention(F, the least alignment of xl, xr, att, out); stats 8-byte aligned. drop may be null.
hipError_t launch_gatv2_attention(const int32_t* rowptr, const int32_t* colind, const float* xl, const float* xr, const float* att,
                                  float* out, float* stats, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope,
                                  const Gatv2AttentionLaunch& r, const EdgeDropout* drop, hipStream_t st);

// The same limits; r for the least alignment of xl, xr, att, out, grad_out, grad_xl and att_part. att_part may be null.
hipError_t launch_gatv2_attention_backward_row(const int32_t* rowptr, const int32_t* colind, const float* xl, const float* xr,
                                               const float* att, const float* stats, const float* out, const float* grad_out, float* delta,
                                               float* grad_xl, float* att_part, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz,
                                               float slope, const Gatv2AttentionLaunch& r, const EdgeDropout* drop, hipStream_t st);

// (colptr [K + 1], rowind within [0, M)); r for the least alignment of xl, xr, att, grad_out and grad_xr.
hipError_t launch_gatv2_attention_backward_col(const int32_t* colptr, const int32_t* rowind, const float* xl, const float* xr,
                                               const float* att, const float* stats, const float* delta, const float* grad_out,
                                               float* grad_xr, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope,
                                               const Gatv2AttentionLaunch& r, const EdgeDropout* drop, hipStream_t st);

}  // namespace gespmm
