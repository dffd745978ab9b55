// sddmm_f32.h — the fp32 operand trait of the SDDMM kernels (sddmm_edge.h, sddmm_heads.h): V floats per load (dword, dwordx2,
// dwordx4), one fmaf per element. Shared by sddmm_kernels.hip and sddmm_heads.hip; the text is the one sddmm_kernels.hip held.
#pragma once

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

}  // namespace gespmm
