// spmm_relational.h — internal interface of the relational aggregate-and-linear on 16-bit features
// (gespmm_csr_spmm_relational_x16; kernel: spmm_relational.hip): an RGCN layer in one kernel.
//
//   H_r[i, :] = narrow( row_scale[r M + i] * sum over the entries e of row r M + i, in CSR order, of val[e] * X[colind[e], :] )   K columns
//   out[i, :] = narrow( sum_r H_r[i, :] @ W[r]^T + X_root[i, :] @ W_root^T + bias )                                         N_out columns
//
// The graph is a STACKED CSR: relation r's row i is row r M + i of one ordinary CSR with R M rows over Kn columns, so the 16-bit product
// on it returns every H_r as it stands (spmm_linear.h: one fp32 chain from +0, one fp32 multiply by row_scale, ONE rounding). No H_r
// leaves the workgroup: each goes through the one LDS tile and all of them accumulate into the same matrix-unit accumulators. W is
// [R, N_out, K] row-major and W_root [N_out, K]. The GEMM accumulates in fp32 in the hardware's order; bias is one fp32 add and the
// store rounds once.
#pragma once
#include "spmm_linear.h"

namespace gespmm {

struct SpmmRelationalArgs {
    const int32_t* rowptr;   // [R M + 1]
    const int32_t* colind;   // [nnz]
    const float* val;        // [nnz] or NULL: A == 1 on its pattern
    const float* row_scale;  // [R M] or NULL
    const float* X;          // [Kn, K] 16-bit elements, seen as words
    const void* W;           // [R, N_out, K]
    const void* Xroot;       // [M, K] or NULL
    const void* Wroot;       // [N_out, K] or NULL (with Xroot)
    const float* bias;       // [N_out] or NULL
    void* out;               // [M, N_out]
    int32_t R, M, K, N_out;
};

// The sizes every route of the op takes: GESPMM_EINVAL / GESPMM_ERANGE codes as plain ints (-1 / -3), 0 when fine. Every product is
// formed by division: R M, Kn, nnz, R M K (the composition's aggregate), Kn K, M N_out and R N_out K are 32-bit element positions.
inline int spmm_relational_sizes(int64_t R, int64_t M, int64_t Kn, int64_t K, int64_t N_out, int64_t nnz) {
    if (R < 0 || M < 0 || Kn < 0 || K < 0 || N_out < 0 || nnz < 0) return -1;
    const int64_t lim = kLinearMaxWords;
    if (R > lim || M > lim || Kn > lim || nnz > lim || K > lim || N_out > lim) return -3;
    if (R != 0 && M > lim / R) return -3;
    const int64_t RM = R * M;
    if (K != 0 && (RM > lim / K || Kn > lim / K)) return -3;
    if (N_out != 0 && (M > lim / N_out || R > lim / N_out || (K != 0 && R * N_out > lim / K))) return -3;
    return 0;
}

// Does the kernel serve this shape? `align`: the largest power of two (<= 16) that divides the address of every 16-bit array.
// The one decision behind gespmm_spmm_relational_route_x16 and the launch of gespmm_csr_spmm_relational_x16.
inline bool spmm_relational_served(int64_t R, int64_t M, int64_t Kn, int64_t K, int64_t N_out, int64_t nnz, int align) {
    if (spmm_relational_sizes(R, M, Kn, K, N_out, nnz) != 0 || M == 0 || R < 1) return false;
    return K % 8 == 0 && K >= 8 && K <= kLinearMaxK && N_out >= 1 && N_out <= kLinearMaxNOut && align >= 16;
}

// hipErrorInvalidValue where the shape is not served or dtype is neither kX16F16 nor kX16Bf16.
hipError_t launch_spmm_relational_x16(const SpmmRelationalArgs& a, int dtype, hipStream_t st);

}  // namespace gespmm
