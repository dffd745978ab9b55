// spmm_relational_wgrad.h — internal interface of the fused relational weight gradient on 16-bit features
// (gespmm_csr_spmm_relational_wgrad_x16; kernels: spmm_relational_wgrad.hip): the backward of an RGCN layer's weights without the
// [R M, K] stack of aggregates.
//
//   H_r[i, :]  = narrow( row_scale[r M + i] * sum over the entries e of row r M + i, in CSR order, of val[e] * X[colind[e], :] )   (never stored)
//   grad_W[r]  = narrow( sum_i grad_out[i, :]^T H_r[i, :] )                                          [R, N_out, K], fp32 sums, ONE rounding
//
// H_r is spmm_relational.h's (the 16-bit product's bits) and exists only as one transposed 64-row, 64-column LDS tile at a time. The
// reduction runs over ROWS: a workgroup owns one (K-slab, relation, row chunk), keeps the [N_out, 64] partial in matrix-unit
// accumulators across its chunk and writes it to partials[c][r][n][k] in fp32; a second kernel adds the C partials in the order
// c = 0 .. C - 1 and rounds once. No atomics: the same inputs and the same C give the same bits.
#pragma once
#include <algorithm>

#include "spmm_relational.h"

namespace gespmm {

constexpr int kWgradSlab = 64;            // columns of X per K-slab: two 32-column MFMA tiles
constexpr int kWgradStride = 64 + 8;      // elements between rows of the transposed tiles HT[k][i], GT[n][i] (16 bytes of padding)
constexpr int64_t kWgradWorkgroups = 1024;  // about four workgroups on each of the 256 compute units

struct SpmmRelationalWgradArgs {
    const int32_t* rowptr;   // [R M + 1]
    const int32_t* colind;   // [nnz]
    const float* val;        // [nnz] or NULL: A == 1 on its pattern
    const float* row_scale;  // [R M] or NULL
    const float* X;          // [Kn, K] 16-bit elements, seen as words
    const void* grad_out;    // [M, N_out]
    float* partials;         // [C, R, N_out, K] fp32, the caller's
    void* grad_w;            // [R, N_out, K]
    int32_t R, M, K, N_out, C;
};

inline int64_t spmm_relational_wgrad_blocks(int64_t M) { return (M + kLinearBlockRows - 1) / kLinearBlockRows; }

// The chunk count the library picks (sizes already through spmm_relational_sizes): the smallest C that fills the machine,
// ceil(1024 / (R slabs)), capped by the 64-row blocks there are, by a workspace of at most half the [R M, K] 16-bit stack the kernel
// exists to avoid (C R N_out K 4 <= R M K 2 / 2, i.e. C <= M / (4 N_out)). Never below 1. The last cap keeps the workspace inside
// 32-bit positions wherever C > 1: C R N_out K <= R M K / 4.
inline int64_t spmm_relational_wgrad_chunks(int64_t R, int64_t M, int64_t K, int64_t N_out) {
    if (R == 0 || M == 0 || K == 0 || N_out == 0) return 0;
    const int64_t slabs = (K + kWgradSlab - 1) / kWgradSlab;
    int64_t C = (kWgradWorkgroups + R * slabs - 1) / (R * slabs);
    C = std::min(C, spmm_relational_wgrad_blocks(M));
    C = std::min(C, M / (4 * N_out));
    return std::max<int64_t>(C, 1);
}

// Does the kernel serve this shape with C chunks? spmm_relational_served's shapes, 1 <= C <= ceil(M / 64) and a workspace of 32-bit
// element positions. The one decision behind gespmm_spmm_relational_wgrad_route_x16 and the launch.
inline bool spmm_relational_wgrad_served(int64_t R, int64_t M, int64_t Kn, int64_t K, int64_t N_out, int64_t nnz, int64_t C, int align) {
    if (!spmm_relational_served(R, M, Kn, K, N_out, nnz, align)) return false;
    return C >= 1 && C <= spmm_relational_wgrad_blocks(M) && C <= kLinearMaxWords / (R * N_out * K);
}

// hipErrorInvalidValue where the shape is not served or dtype is neither kX16F16 nor kX16Bf16. Two launches on `st`, no allocation.
hipError_t launch_spmm_relational_wgrad_x16(const SpmmRelationalWgradArgs& a, int dtype, hipStream_t st);

}  // namespace gespmm
