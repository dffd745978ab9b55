// spmm_linear.h — internal interface of the fused aggregate-and-linear on 16-bit features (gespmm_csr_spmm_linear_x16; kernel:
// spmm_linear.hip):
//
//   H[r, :]   = narrow( row_scale[r] * sum over the entries e of row r, in CSR order, of val[e] * X[colind[e], :] )      K columns
//   out[r, :] = narrow( H[r, :] @ W_n^T + X_root[r, :] @ W_r^T + bias )                                              N_out columns
//
// H is the 16-bit product as it stands (spmm_stream.h with HalfSpmmArgs: one fp32 fma / add chain per element from +0, one fp32
// multiply by row_scale, ONE rounding) and never leaves the workgroup: 64 rows of it live in LDS and feed the matrix unit. W_n and W_r
// are [N_out, K] row-major, torch.nn.Linear's layout. The GEMM accumulates in fp32 in the hardware's order; bias is one fp32 add, and
// the store rounds once.
#pragma once
#include "spmm_kernels.h"

namespace gespmm {

constexpr int kLinearBlockRows = 64;  // rows of H per workgroup: two 32-row MFMA tiles
constexpr int kLinearMaxK = 256;      // LDS tile: 64 x (2 K_pad + 16) bytes <= 33 KB
constexpr int kLinearMaxNOut = 256;   // eight 32-column slabs, two per wavefront
constexpr int64_t kLinearMaxWords = 0x7fffffffLL - 4096;  // 32-bit element positions, as everywhere (kSddmmMaxNnz)

struct SpmmLinearArgs {
    const int32_t* rowptr;
    const int32_t* colind;
    const float* val;        // [nnz] or NULL: A == 1 on its pattern
    const float* row_scale;  // [M] or NULL
    const float* X;          // [Kn, K] 16-bit elements, seen as words
    const void* W;           // [N_out, K]: W_n
    const void* Xroot;       // [M, K] or NULL
    const void* Wroot;       // [N_out, K] or NULL (with Xroot): W_r
    const float* bias;       // [N_out] or NULL
    void* out;               // [M, N_out]
    int32_t M, K, N_out;
};

// The sizes every route of the op takes: GESPMM_EINVAL / GESPMM_ERANGE codes as plain ints (-1 / -3), 0 when fine.
inline int spmm_linear_sizes(int64_t M, int64_t Kn, int64_t K, int64_t N_out, int64_t nnz) {
    if (M < 0 || Kn < 0 || K < 0 || N_out < 0 || nnz < 0) return -1;
    const int64_t lim = kLinearMaxWords;
    if (M > lim || Kn > lim || nnz > lim || K > lim || N_out > lim) return -3;
    if ((K != 0 && (M > lim / K || Kn > lim / K)) || (N_out != 0 && M > lim / N_out)) return -3;
    return 0;
}

// Does the kernel serve this shape? `align`: the largest power of two (<= 16) that divides the address of every 16-bit array.
// The one decision behind gespmm_spmm_linear_route_x16 and the launch of gespmm_csr_spmm_linear_x16.
inline bool spmm_linear_served(int64_t M, int64_t Kn, int64_t K, int64_t N_out, int64_t nnz, int align) {
    if (spmm_linear_sizes(M, Kn, K, N_out, nnz) != 0 || M == 0) return false;
    return K % 8 == 0 && K >= 8 && K <= kLinearMaxK && N_out >= 1 && N_out <= kLinearMaxNOut && align >= 16;
}

// hipErrorInvalidValue where the shape is not served or dtype is neither kX16F16 nor kX16Bf16.
hipError_t launch_spmm_linear_x16(const SpmmLinearArgs& a, int dtype, hipStream_t st);

}  // namespace gespmm
