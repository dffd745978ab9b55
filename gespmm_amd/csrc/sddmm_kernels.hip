// sddmm_kernels.hip — sampled dense-dense product on a sparse pattern (gfx950), fp32 operands.
//
//     out[e] = sum_{j < N} D1[row(e), j] * D2[col(e), j]        (pattern order)
//
// The kernels, their launch forms and the summation order they pin are in sddmm_edge.h, written once for every operand type;
// this file is the fp32 operand (sddmm_f32.h: V floats per load — dword, dwordx2, dwordx4 — one fmaf per element) and its entry point.
// The 16-bit operands are in sddmm_x16.hip.

#include "sddmm_edge.h"
#include "sddmm_f32.h"

namespace gespmm {

hipError_t launch_sddmm(const int32_t* rows, bool csr, const int32_t* colind, const float* D1, const float* D2,
                        float* out, int64_t M, int64_t nnz, int64_t N, hipStream_t st) {
    return launch_sddmm_op<SddmmF32>(rows, csr, colind, D1, D2, out, M, nnz, N, st);
}

}  // namespace gespmm
