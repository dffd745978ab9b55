// spmm_tile_mfma.h — what the aggregate-and-linear kernels share without a change to their code: the matrix-instruction wrapper, the
// fp32 register barrier and the two launch dispatchers (spmm_linear.hip, spmm_relational.hip, spmm_relational_wgrad.hip,
// spmm_relational_f32.hip). Internal: included by those four files only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "spmm_device.h"

namespace gespmm {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// v_mfma_f32_32x32x16_{f16,bf16}: lane l holds, of A, row l % 32 and the 8 consecutive k of half l / 32; of B, column l % 32 and the
// same 8 k; of the 32 x 32 result, column l % 32 and rows 8 (v / 4) + 4 (l / 32) + v % 4 in register v.
template <int DT>
__device__ __forceinline__ floatx16 mfma_32x32x16(uint4 a, uint4 b, floatx16 c) {
    if constexpr (DT == kX16F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(halfx8, a), __builtin_bit_cast(halfx8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// x as a finished fp32 value in a register. Without it the compiler merges an fp32 multiply (or add) with the fp16 rounding behind it
// into ONE operation that rounds the exact result straight to fp16 (v_fma_mixlo_f16): the fp32 rounding skipped, and an element that
// differs from the 16-bit product's wherever fl32 lands on an fp16 tie.
__device__ __forceinline__ float fl32(float x) {
    asm volatile("" : "+v"(x));
    return x;
}

// f(W, WPL) as integral constants: the smallest lane group (4 .. 64 lanes) that covers the `units` words / vectors of a row, two per
// lane beyond 64. MAX_UNITS, the most the kernel serves, bounds the geometries that are instantiated.
template <int MAX_UNITS, typename F>
hipError_t dispatch_lane_group(int units, F f) {
    using std::integral_constant;
    if constexpr (MAX_UNITS > 64)
        if (units > 64) return f(integral_constant<int, 64>{}, integral_constant<int, 2>{});
    if constexpr (MAX_UNITS > 32)
        if (units > 32) return f(integral_constant<int, 64>{}, integral_constant<int, 1>{});
    if (units > 16) return f(integral_constant<int, 32>{}, integral_constant<int, 1>{});
    if (units > 8) return f(integral_constant<int, 16>{}, integral_constant<int, 1>{});
    if (units > 4) return f(integral_constant<int, 8>{}, integral_constant<int, 1>{});
    return f(integral_constant<int, 4>{}, integral_constant<int, 1>{});
}

// f(DT, VALUED) as integral constants; hipErrorInvalidValue where dtype is neither kX16F16 nor kX16Bf16.
template <typename F>
hipError_t dispatch_x16_valued(int dtype, bool valued, F f) {
    using std::integral_constant;
    if (dtype == kX16F16) return valued ? f(integral_constant<int, kX16F16>{}, std::true_type{}) : f(integral_constant<int, kX16F16>{}, std::false_type{});
    if (dtype == kX16Bf16) return valued ? f(integral_constant<int, kX16Bf16>{}, std::true_type{}) : f(integral_constant<int, kX16Bf16>{}, std::false_type{});
    return hipErrorInvalidValue;
}

}  // namespace gespmm
