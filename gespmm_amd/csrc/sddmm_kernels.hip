// sddmm_kernels.hip — sampled dense-dense product on a sparse pattern (gfx950), fp32 operands.
//
//     out[e] = sum_{j < N} D1[row(e), j] * D2[col(e), j]        (pattern order)
//
// The kernels, their launch forms and the summation order they pin are in sddmm_edge.h, written once for every operand type;
// this file is the fp32 operand — V floats per load (dword, dwordx2, dwordx4), one fmaf per element — and its entry point.
// The 16-bit operands are in sddmm_x16.hip.

#include "sddmm_edge.h"

namespace gespmm {

template <int V> struct SdVec;
template <> struct SdVec<1> { using type = float; };
template <> struct SdVec<2> { using type = float __attribute__((ext_vector_type(2))); };
template <> struct SdVec<4> { using type = float __attribute__((ext_vector_type(4))); };

struct SddmmF32 {
    using elem = float;
    static constexpr int kMaxV = 4;
    template <int V> using vec = typename SdVec<V>::type;
    // vectors per lane that cover a row: a lane walks ~32 bytes of each row, at most 8 loads
    template <int V> static constexpr int it() { return (V == 4) ? 2 : (V == 2) ? 4 : 8; }
    template <int V> static __device__ __forceinline__ float dot(vec<V> x, vec<V> y, float acc) {
        if constexpr (V == 1) {
            acc = __builtin_fmaf(x, y, acc);
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i) acc = __builtin_fmaf(x[i], y[i], acc);
        }
        return acc;
    }
};

hipError_t launch_sddmm(const int32_t* rows, bool csr, const int32_t* colind, const float* D1, const float* D2,
                        float* out, int64_t M, int64_t nnz, int64_t N, hipStream_t st) {
    return launch_sddmm_op<SddmmF32>(rows, csr, colind, D1, D2, out, M, nnz, N, st);
}

}  // namespace gespmm
