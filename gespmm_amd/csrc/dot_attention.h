// dot_attention.h — fused scaled dot-product attention over the entries of a sparsity pattern, and its backward
// (gespmm_dot_attention_f32, gespmm_dot_attention_backward_q_f32, gespmm_dot_attention_backward_kv_f32 and their *_dropout_f32 forms;
// kernels: dot_attention.hip). fp32, no plan, no composition route, no environment pin.
//
// q is [M, H, F] (the aggregating node: the row of an entry), k and v are [K, H, F] (the neighbour: the column); out and grad_out are
// [M, H, F], stats is [M, H, 2], delta is [M, H]. For entry p of row r with column c and head h:
//   s_p        = fl(scale * dot(q[r, h, :], k[c, h, :]))
//   a_p        = exp(s_p - m) / l            m = max_p s_p,  l = sum_p exp(s_p - m)            stats[r, h] = (m, l)
//   out[r,h,:] = sum_p a_p v[c, h, :]
// Nothing of size nnz is read, written or allocated apart from the index arrays, in either direction.
//
// GEOMETRY, all three kernels. The unit of work is the (segment, head) pair: segments are the rows in the forward and the q-pass, the
// columns in the k/v-pass. A group of W lanes owns a pair; the 64 / W groups of a wavefront take consecutive pairs; a wavefront past
// the end returns whole. The lanes of a group are contiguous in f, V floats per load, 8 floats per lane and operand: (V, W) =
// resolve_dot_attention(F, alignment) — resolve_sddmm's rule at WIDTH F: V the widest of 4 / 2 / 1 that divides F and whose bytes divide
// every dense operand's address (no vector spans two heads), W the smallest power of two in 4 .. 64 with 8 W >= F. F > 512 is NOT
// SERVED (kDotAttentionMaxF): the entry points answer GESPMM_ERR_UNSUPPORTED and launch nothing. The segment's own slices (q, or k and
// v) and all accumulators live in registers for the whole segment. The group reads W indices at a time, coalesced, and broadcasts them;
// the gathers of two entries, both operands, are requested before the first is used. A hub segment is walked by its one lane group
// (a limit, as in gatv2_score.h).
//
// PINNED ORDERS.
//   dot(x, y): lane l runs ONE chain acc = fmaf(x_j, y_j, acc) from +0 over j = l V + i + t W V (i ascending inside a vector, t ascending
//   below ceil(F / (W V))), then the xor butterfly W/2 .. 1. A lane past the slice contributes fmaf(0, 0, acc). fmaf(a, b, acc) commutes
//   in a and b, so the row pass and the column pass compute THE SAME BITS of s_p and g_p.
//   Every per-word accumulation is one chain per output word in segment (entry) order. The head, H, alignment, capture and run leave
//   no trace beyond V (which moves the dot's lane positions).
//
// FORWARD (rowptr, colind -> out, stats). One sweep over the row with an online softmax; per entry, in entry order:
//   m' = fmaxf(m, s_p);  c = __expf(m - m');  t = __expf(s_p - m');  l = fmaf(l, c, t);  acc_f = fmaf(t, v_f, fl(acc_f * c));  m = m'
// The first entry starts from m = s_p, l = 0, acc = 0, which gives m = s_p, l = 1, acc = v with no exp(-inf - ..) (__expf(0) == 1).
// out = acc / l; (m, l) is one 8-byte store per pair. Every word of out and stats is written: an empty row writes +0 everywhere.
//
// BACKWARD, ROW PASS (rowptr, colind; reads q, k, v, stats, out, grad_out; writes delta, grad_q):
//   delta[r, h]     = dot(grad_out[r, h, :], out[r, h, :])
//   a_p = __expf(s_p - m) / l        g_p = dot(grad_out[r, h, :], v[c, h, :])        ds_p = a_p * (g_p - delta)
//   grad_q[r, h, f] = fl(scale * chain over p of fmaf(ds_p, k[c, h, f], acc))
// BACKWARD, COLUMN PASS (colptr, rowind — no csc_order; reads q, k, v, stats, delta, grad_out; writes grad_k, grad_v). Column c's k and
// v slices are held; per entry with row r the pass gathers q[r, h, :], grad_out[r, h, :], stats[r, h] and delta[r, h]; s_p, a_p, g_p and
// ds_p have the bits of the row pass.
//   grad_k[c, h, f] = fl(scale * chain over p of fmaf(ds_p, q[r, h, f], acc))        grad_v[c, h, f] = chain of fmaf(a_p, grad_out[r, h, f], acc)
//
// DROPOUT on the coefficients (drop != nullptr; edge_dropout.h: keep is a function of (seed, r, c, h), so the entries of a multigraph
// with the same (row, column) share it). Forward: l sums every entry, acc takes fl(t * keep_scale) for a kept entry and +0 for a
// dropped one. Backward: g_p becomes g'_p = fl(g_p * keep_scale) or +0 directly after its chain, delta stays dot(grad_out, out), grad_v
// uses fl(a_p * keep_scale) or +0.
//
// Safety rules: every load is clamped to a valid word and dropped by a select, trip counts are wave-uniform, only stores
// are predicated. No atomics, no workspace, no allocation, no host synchronisation: all launches are capturable.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edge_dropout.h"
#include "select.h"

namespace gespmm {

// M, K, H, F, nnz >= 1; F <= kDotAttentionMaxF; nnz, M H F, K H F and 2 M H <= kSddmmMaxNnz (32-bit word positions); colind within [0, K);
// r = resolve_dot_attention(F, the least alignment of q, k, v, out); stats 8-byte aligned. drop may be null.
hipError_t launch_dot_attention(const int32_t* rowptr, const int32_t* colind, const float* q, const float* k, const float* v, float* out,
                                float* stats, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale,
                                const DotAttentionLaunch& r, const EdgeDropout* drop, hipStream_t st);

// The same limits; r for the least alignment of q, k, v, out, grad_out and grad_q.
hipError_t launch_dot_attention_backward_q(const int32_t* rowptr, const int32_t* colind, const float* q, const float* k, const float* v,
                                           const float* stats, const float* out, const float* grad_out, float* delta, float* grad_q,
                                           int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, const DotAttentionLaunch& r,
                                           const EdgeDropout* drop, hipStream_t st);

// (colptr [K + 1], rowind within [0, M)); r for the least alignment of q, k, v, grad_out, grad_k and grad_v.
hipError_t launch_dot_attention_backward_kv(const int32_t* colptr, const int32_t* rowind, const float* q, const float* k, const float* v,
                                            const float* stats, const float* delta, const float* grad_out, float* grad_k, float* grad_v,
                                            int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, const DotAttentionLaunch& r,
                                            const EdgeDropout* drop, hipStream_t st);

}  // namespace gespmm
