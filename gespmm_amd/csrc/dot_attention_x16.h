// dot_attention_x16.h — the fused dot-product attention of dot_attention.h and its backward on 16-bit node terms
// (gespmm_dot_attention_x16, gespmm_dot_attention_backward_q_x16, gespmm_dot_attention_backward_kv_x16 and their *_dropout_x16 forms;
// kernels: dot_attention_x16.hip). No plan, no composition route, no environment pin.
//
// OPERANDS. q, out, grad_out, grad_q [M, H, F] and k, v, grad_k, grad_v [K, H, F] are IEEE fp16 or bfloat16 (dtype kX16F16 / kX16Bf16,
// one type per call). stats [M, H, 2], delta [M, H] and scale stay fp32: the row statistics and what every entry's coefficient is taken
// from.
//
// ARITHMETIC: dot_attention.h's, expression for expression. Every 16-bit element is widened exactly at its use (widen_x16,
// spmm_device.h; subnormals included); the pinned lane dot is ONE fmaf chain per lane from +0, then the xor butterfly;
// s_p = fl(scale * dot), the online softmax m' / c / t / l / acc, out = acc / l, a_p, g_p, ds_p, the per-word chains in entry order and
// the dropout placement (fl(t * keep_scale), g'_p, fl(a_p * keep_scale)) are the fp32 kernels'; every accumulation is fp32. The row
// pass reads the STORED, 16-bit out for delta = dot(grad_out, out). Every 16-bit result is rounded ONCE, at its store (narrow_x16: to
// nearest even, overflow to +-inf, NaN stays NaN); for grad_q and grad_k that is fl32(scale * chain), then one rounding. No packed-fp16
// arithmetic and no dot2: they round differently.
//
// GEOMETRY: the fp32 kernel's with V counted in ELEMENTS. V in {4, 2, 1}: an 8 / 4 / 2-byte load; 8 elements per lane and operand; W
// the smallest power of two in 4 .. 64 with 8 W >= F; V the widest of 4 / 2 / 1 that divides F and whose 2 V bytes divide the address of
// every 16-bit operand and result of the launch (resolve_dot_attention_x16, select.cpp). F > 512 is NOT SERVED: the entry points answer
// GESPMM_ERR_UNSUPPORTED and launch nothing. A 16-byte load form (V = 8, one vector per lane) is deliberately NOT built: it moves the
// lane positions of the dots and would cost the property below.
//
// THE PROPERTY. Lane positions, chains and orders are those of the fp32 kernels at the same (V, W). Wherever
// gespmm_describe_dot_attention answers the same (V, W) for the widened operands — a 16-bit operand b bytes off a 16-byte boundary
// corresponds to an fp32 operand 2 b bytes off — stats and delta have the BITS of the fp32 entry points on the widened operands (the
// row pass fed widen(out16), the column pass fed that delta), and out, grad_q, grad_k and grad_v are those calls' results narrowed once.
//
// GATHERS IN FLIGHT: two entries, both operands each — kDaUnroll of dot_attention.hip, CARRIED OVER, NOT MEASURED on 16-bit rows. A
// gathered vector stays packed in its registers (V / 2 words; one at V = 1) until it is widened: the four gathered rows of a step are 16
// registers where the fp32 kernel holds 32.
//
// Limits are in ELEMENT positions: M H F, K H F, nnz, nnz H and 2 M H <= kSddmmMaxNnz. Safety rules, unchanged: every load
// is clamped to a valid element and dropped by a select, trip counts are wave-uniform, only stores are predicated, a wavefront past the
// end returns whole, an empty segment writes +0 to every word. No atomics, no workspace, no allocation, no host synchronisation: all
// launches are capturable. Plain C++ / HIP, no inline assembly.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edge_dropout.h"
#include "select.h"

namespace gespmm {

// The limits of launch_dot_attention in element positions; r = resolve_dot_attention_x16(F, the least alignment of q, k, v and out);
// stats 8-byte aligned. drop may be null. dtype: kX16F16 / kX16Bf16.
hipError_t launch_dot_attention_x16(const int32_t* rowptr, const int32_t* colind, const void* q, const void* k, const void* v, void* out,
                                    float* stats, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale,
                                    const DotAttentionLaunch& r, const EdgeDropout* drop, hipStream_t st);

// r for the least alignment of q, k, v, out, grad_out and grad_q.
hipError_t launch_dot_attention_backward_q_x16(const int32_t* rowptr, const int32_t* colind, const void* q, const void* k, const void* v,
                                               const float* stats, const void* out, const void* grad_out, float* delta, void* grad_q,
                                               int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale,
                                               const DotAttentionLaunch& r, const EdgeDropout* drop, hipStream_t st);

// (colptr [K + 1], rowind within [0, M)); r for the least alignment of q, k, v, grad_out, grad_k and grad_v.
hipError_t launch_dot_attention_backward_kv_x16(const int32_t* colptr, const int32_t* rowind, const void* q, const void* k, const void* v,
                                                const float* stats, const float* delta, const void* grad_out, void* grad_k, void* grad_v,
                                                int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale,
                                                const DotAttentionLaunch& r, const EdgeDropout* drop, hipStream_t st);

}  // namespace gespmm
