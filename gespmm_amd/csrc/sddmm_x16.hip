// sddmm_x16.hip — SDDMM on 16-bit dense operands (IEEE fp16 / bfloat16 D1 and D2 of the same type, fp32 out; gfx950).
//
//     out[e] = sum_{j < N} widen(D1[row(e), j]) * widen(D2[col(e), j])        (pattern order)
//
// The kernels of sddmm_edge.h with the operand trait SddmmX16<DT>: a lane's register vector holds V elements as V / 2 32-bit
// words (dword, dwordx2, dwordx4 loads for V = 2, 4, 8; V = 1 is one ushort), and every element is widened — exactly, subnormals
// included (widen_x16, spmm_device.h) — at its FMA. The arithmetic is the fp32 kernels': one fmaf per element in element order
// (the low half of a word is the earlier element), then the xor butterfly. No dot2 instruction and no packed-fp16 arithmetic:
// they round differently. The product of two fp16 or two bf16 numbers is exact in fp32, so what rounds is the chain of adds, and
// the bits depend on (V, W) alone — resolve_sddmm at element size 2: V up to 8, a V = 8 edge in the registers a V = 4 fp32 edge has.
// There is no composition route: every N and every 2-byte aligned address runs one of these kernels, and the only temporary is
// the blocked form's split points.
//
// The multi-head form (gespmm_sddmm_{coo,csr}_heads_x16) is the kernel of sddmm_heads.h on the same trait: head h has the bits of the
// single-head call above on the contiguous copies of its slices, at the same (V, W).

#define GESPMM_SDDMM_HEADS_KERNELS
#include "sddmm_heads.h"

#include "sddmm_edge.h"
#include "spmm_device.h"

namespace gespmm {

template <int V> struct SdWords;
template <> struct SdWords<1> { using type = uint16_t; };
template <> struct SdWords<2> { using type = uint32_t; };
template <> struct SdWords<4> { using type = uint32_t __attribute__((ext_vector_type(2))); };
template <> struct SdWords<8> { using type = uint32_t __attribute__((ext_vector_type(4))); };

template <int DT>
struct SddmmX16 {
    using elem = uint16_t;
    static constexpr int kMaxV = 8;
    template <int V> using vec = typename SdWords<V>::type;
    // vectors per lane that cover a row: a lane walks ~32 bytes of each row, at most 8 loads
    template <int V> static constexpr int it() { return (V == 8) ? 2 : (V == 4) ? 4 : 8; }
    static __device__ __forceinline__ float pair(uint32_t xw, uint32_t yw, float acc) {
        float x0, x1, y0, y1;
        widen_x16<DT>(__uint_as_float(xw), x0, x1);
        widen_x16<DT>(__uint_as_float(yw), y0, y1);
        acc = __builtin_fmaf(x0, y0, acc);
        return __builtin_fmaf(x1, y1, acc);
    }
    template <int V> static __device__ __forceinline__ float dot(vec<V> x, vec<V> y, float acc) {
        if constexpr (V == 1) {
            float x0, x1, y0, y1;
            widen_x16<DT>(__uint_as_float((uint32_t)x), x0, x1);
            widen_x16<DT>(__uint_as_float((uint32_t)y), y0, y1);
            acc = __builtin_fmaf(x0, y0, acc);
        } else if constexpr (V == 2) {
            acc = pair(x, y, acc);
        } else {
#pragma unroll
            for (int i = 0; i < V / 2; ++i) acc = pair(x[i], y[i], acc);
        }
        return acc;
    }
};

hipError_t launch_sddmm_x16(const int32_t* rows, bool csr, const int32_t* colind, const void* D1, const void* D2, float* out,
                            int dtype, int64_t M, int64_t nnz, int64_t N, hipStream_t st) {
    const uint16_t* d1 = static_cast<const uint16_t*>(D1);
    const uint16_t* d2 = static_cast<const uint16_t*>(D2);
    if (dtype == kX16F16) return launch_sddmm_op<SddmmX16<kX16F16>>(rows, csr, colind, d1, d2, out, M, nnz, N, st);
    if (dtype == kX16Bf16) return launch_sddmm_op<SddmmX16<kX16Bf16>>(rows, csr, colind, d1, d2, out, M, nnz, N, st);
    return hipErrorInvalidValue;
}

hipError_t launch_sddmm_heads_x16(const int32_t* rows, const int32_t* colind, const void* D1, const void* D2, float* out, int dtype,
                                  int64_t M, int64_t nnz, int64_t H, int64_t F, const SddmmHeadsLaunch& r, hipStream_t st) {
    const uint16_t* d1 = static_cast<const uint16_t*>(D1);
    const uint16_t* d2 = static_cast<const uint16_t*>(D2);
    if (dtype == kX16F16) return launch_sddmm_heads_op<SddmmX16<kX16F16>>(rows, colind, d1, d2, out, M, nnz, H, F, r, st);
    if (dtype == kX16Bf16) return launch_sddmm_heads_op<SddmmX16<kX16Bf16>>(rows, colind, d1, d2, out, M, nnz, H, F, r, st);
    return hipErrorInvalidValue;
}

}  // namespace gespmm
