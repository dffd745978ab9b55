// spmm_relational_f32.h — internal interface of the relational aggregate-and-linear on fp32 features
// (gespmm_csr_spmm_relational_f32; kernel: spmm_relational_f32.hip): an RGCN layer in one kernel, R = 1 the plain aggregate-and-linear.
//
//   H_r[i, :] = fl32( row_scale[r M + i] * sum over the entries e of row r M + i, in CSR order, of val[e] * X[colind[e], :] )   K columns
//   out[i, :] = sum_r H_r[i, :] @ W[r]^T + X_root[i, :] @ W_root^T + bias                                                  N_out columns
//
// The graph is the STACKED CSR of spmm_relational.h, and H_r has the bits of the fp32 product on it (gespmm_csr_spmm_f32: one fp32 chain
// from +0 — fmaf(val, x, acc), or acc + x without val — then one fp32 multiply by row_scale). No H_r leaves the workgroup: each goes
// through the one fp32 LDS tile and all of them accumulate into the same accumulators of v_mfma_f32_32x32x2_f32, in the hardware's and
// the kernel's order (fixed, not pinned). W is [R, N_out, K] row-major and W_root [N_out, K]; bias is one fp32 add.
#pragma once
#include "spmm_relational.h"

namespace gespmm {

constexpr int kRelF32MaxK = 256;     // LDS tile: 64 x (K_pad + 4) floats <= 66 560 bytes
constexpr int kRelF32MaxNOut = 256;  // eight 32-column slabs, two per wavefront

struct SpmmRelationalF32Args {
    const int32_t* rowptr;   // [R M + 1]
    const int32_t* colind;   // [nnz]
    const float* val;        // [nnz] or NULL: A == 1 on its pattern
    const float* row_scale;  // [R M] or NULL
    const float* X;          // [Kn, K]
    const float* W;          // [R, N_out, K]
    const float* Xroot;      // [M, K] or NULL
    const float* Wroot;      // [N_out, K] or NULL (with Xroot)
    const float* bias;       // [N_out] or NULL
    float* out;              // [M, N_out]
    int32_t R, M, K, N_out;
};

// Does the kernel serve this shape? `align`: the largest power of two (<= 16) that divides the address of X, W, X_root, W_root and out.
// The one decision behind gespmm_spmm_relational_route_f32 and the launch of gespmm_csr_spmm_relational_f32.
inline bool spmm_relational_f32_served(int64_t R, int64_t M, int64_t Kn, int64_t K, int64_t N_out, int64_t nnz, int align) {
    if (spmm_relational_sizes(R, M, Kn, K, N_out, nnz) != 0 || M == 0 || R < 1) return false;
    return K % 4 == 0 && K >= 4 && K <= kRelF32MaxK && N_out >= 1 && N_out <= kRelF32MaxNOut && align >= 16;
}

// hipErrorInvalidValue where the shape is not served.
hipError_t launch_spmm_relational_f32(const SpmmRelationalF32Args& a, hipStream_t st);

}  // namespace gespmm
