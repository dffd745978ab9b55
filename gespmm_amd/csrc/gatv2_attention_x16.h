// gatv2_attention_x16.h — the fused GATv2 attention of gatv2_attention.h and its backward on 16-bit node terms
// (gespmm_gatv2_attention_x16, gespmm_gatv2_attention_backward_row_x16, gespmm_gatv2_attention_backward_col_x16 and their *_dropout_x16
// forms; kernels: gatv2_attention_x16.hip). No plan, no composition route, no environment pin.
//
// OPERANDS. xl [M, H, F], xr [K, H, F], out, grad_out, grad_xl [M, H, F] and grad_xr [K, H, F] are IEEE fp16 or bfloat16 (dtype kX16F16 /
// kX16Bf16, one type per call). att [H, F], stats [M, H, 2], delta [M, H] and att_part [M, H, F] stay fp32: parameters, row statistics
// and everything a sum over nodes is taken of — the split of the 16-bit edge score (gatv2_score.h).
//
// ARITHMETIC: gatv2_attention.h's, expression for expression. Every 16-bit element is widened exactly at its use (widen_x16,
// spmm_device.h; subnormals included); t = fl32(widen(xl_j) + widen(xr_j)) is ONE fp32 add, the leaky branch is t >= 0; the score chain,
// the pinned dot, the xor butterfly and the online softmax are the fp32 kernel's; every accumulation is fp32, in entry order. The row
// pass reads the STORED, 16-bit out for delta = dot(grad_out, out). Every 16-bit result is rounded ONCE, at its store (narrow_x16: to
// nearest even, overflow to +-inf, NaN stays NaN); for grad_xr that is the one add of its two chains, then one rounding. No packed-fp16
// arithmetic and no dot2: they round differently.
//
// GEOMETRY: the fp32 kernel's with V counted in ELEMENTS. V in {4, 2, 1}: an 8 / 4 / 2-byte load of the 16-bit operands, with att's V
// floats at the same element positions; 8 elements per lane and operand; W the smallest power of two in 4 .. 64 with 8 W >= F; V the
// widest of 4 / 2 / 1 that divides F, whose 2 V bytes divide the address of every 16-bit dense operand and result and whose 4 V bytes
// divide the addresses of att and att_part (resolve_gatv2_attention_x16, select.cpp). A 16-byte load form (V = 8, one vector per lane)
// is deliberately NOT built: it moves the lane positions of s_p and the dots and would cost the property below.
//
// THE PROPERTY. Lane positions, chains and orders are those of the fp32 kernels at the same (V, W). Wherever
// gespmm_describe_gatv2_attention answers the same (V, W) for the widened operands — a 16-bit operand b bytes off a 16-byte boundary
// corresponds to an fp32 operand 2 b bytes off — stats, delta and att_part have the BITS of the fp32 entry points on the widened
// operands (the row pass fed widen(out16), the column pass fed that delta), and out, grad_xl and grad_xr are those calls' results
// narrowed once.
//
// GATHERS IN FLIGHT: four entries in the forward and the row pass, two in the column pass — the depths of gatv2_attention.h, CARRIED
// OVER, NOT MEASURED on 16-bit rows. A gathered vector stays packed in its registers (V / 2 words; one at V = 1) until it is widened: the
// four rows of the row passes are 16 registers where the fp32 kernel holds 32.
//
// Limits are in ELEMENT positions: M H F, K H F, nnz, nnz H and 2 M H <= kSddmmMaxNnz. Safety rules, unchanged: every load
// is clamped to a valid element and dropped by a select, trip counts are wave-uniform, only stores are predicated, a wavefront past the
// end returns whole. No atomics, no workspace, no allocation, no host synchronisation: all launches are capturable. Plain C++ / HIP, no
// inline assembly.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edge_dropout.h"
#include "select.h"

namespace gespmm {

// The limits of launch_gatv2_attention in element positions; r = resolve_gatv2_attention_x16(F, the least alignment of xl, xr and out,
// that of att); stats 8-byte aligned. drop may be null. dtype: kX16F16 / kX16Bf16.
hipError_t launch_gatv2_attention_x16(const int32_t* rowptr, const int32_t* colind, const void* xl, const void* xr, const float* att,
                                      void* out, float* stats, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz,
                                      float slope, const Gatv2AttentionLaunch& r, const EdgeDropout* drop, hipStream_t st);

// r for the least alignment of xl, xr, out, grad_out and grad_xl, and the least of att and att_part. att_part may be null.
hipError_t launch_gatv2_attention_backward_row_x16(const int32_t* rowptr, const int32_t* colind, const void* xl, const void* xr,
                                                   const float* att, const float* stats, const void* out, const void* grad_out,
                                                   float* delta, void* grad_xl, float* att_part, int dtype, int64_t M, int64_t K,
                                                   int64_t H, int64_t F, int64_t nnz, float slope, const Gatv2AttentionLaunch& r,
                                                   const EdgeDropout* drop, hipStream_t st);

// (colptr [K + 1], rowind within [0, M)); r for the least alignment of xl, xr, grad_out and grad_xr, and that of att.
hipError_t launch_gatv2_attention_backward_col_x16(const int32_t* colptr, const int32_t* rowind, const void* xl, const void* xr,
                                                   const float* att, const float* stats, const float* delta, const void* grad_out,
                                                   void* grad_xr, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz,
                                                   float slope, const Gatv2AttentionLaunch& r, const EdgeDropout* drop, hipStream_t st);

}  // namespace gespmm
