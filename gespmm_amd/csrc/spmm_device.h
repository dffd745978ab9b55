// spmm_device.h — device-side helpers shared by the kernel translation units (spmm_kernels.hip, spmm_stream_plan.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "spmm_kernels.h"

namespace gespmm {

// ----------------------------------------------------------------------------- small helpers

template <int V> struct VecT;
template <> struct VecT<1> { using type = float; };
template <> struct VecT<2> { using type = float __attribute__((ext_vector_type(2))); };
template <> struct VecT<4> { using type = float __attribute__((ext_vector_type(4))); };

template <int V>
__device__ __forceinline__ void load_vec(float (&dst)[V], const char* base) {
    using T = typename VecT<V>::type;
    T v = *reinterpret_cast<const T*>(base);
    if constexpr (V == 1) {
        dst[0] = v;
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) dst[i] = v[i];
    }
}

template <int V>
__device__ __forceinline__ void load_vec_nt(float (&dst)[V], const char* base) {
    using T = typename VecT<V>::type;
    T v = __builtin_nontemporal_load(reinterpret_cast<const T*>(base));
    if constexpr (V == 1) {
        dst[0] = v;
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) dst[i] = v[i];
    }
}

template <int V, bool NT>
__device__ __forceinline__ void store_vec(float* p, const float (&src)[V]) {
    using T = typename VecT<V>::type;
    T v;
    if constexpr (V == 1) {
        v = src[0];
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] = src[i];
    }
    if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<T*>(p));
    else *reinterpret_cast<T*>(p) = v;
}

// Store with system scope (`sc1`): the line is written through instead of staying in the XCD's L2. C is written once and never
// read by the launch, and in the cache-resident regimes every C line kept in L2 evicts a B row somebody is about to reuse:
// 512-byte rows gathered from a 2 MB table while 1 GB of rows is written run at 25.5 TB/s with plain stores, 27.1 with `nt`,
// 31.3 with `sc1` (31.9 without any store; profiles/r02/l2_gather_steps.log).
template <int V>
__device__ __forceinline__ void store_vec_sc1(float* p, const float (&src)[V]) {
    using T = typename VecT<V>::type;
    T v;
    if constexpr (V == 1) {
        v = src[0];
        asm volatile("global_store_dword %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] = src[i];
        if constexpr (V == 2) asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
        else asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
    }
}

// Workgroup id -> work item id such that XCD x (which receives ids == x mod 8)
// gets a contiguous slice of the item range. Bijective for every n.
__device__ __forceinline__ int xcd_contiguous(int bid, int n) {
    const int q = n >> 3, r = n & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

// Row that owns CSR position q: rowptr[r] <= q < rowptr[r + 1] (behind a run of equal pointers — empty rows — the last of them)
__device__ __forceinline__ int row_of_entry(const int32_t* __restrict__ rowptr, int M, int q) {
    int lo = 0, hi = M;  // rowptr[lo] <= q < rowptr[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rowptr[mid] <= q) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Ordering of a wavefront's own LDS traffic (write by lane i, read by lane j of
// the same wavefront). DS operations of one wavefront execute in issue order, so
// no hardware barrier is needed — only the compiler must keep the order.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}


// CSR stream loads are non-temporal: each entry is used once per launch. (Plain loads
// were measured too — no gain, profiles/r01/kernel_generations_cache_regimes.log.)
template <typename T>
__device__ __forceinline__ T load_csr(const T* p) {
    return __builtin_nontemporal_load(p);
}

template <int RED, bool VALUED>
__device__ __forceinline__ float combine(float acc, float a, float b) {
    if constexpr (RED == kReduceMax) {
        return fmaxf(acc, b);
    } else if constexpr (VALUED) {
        return __builtin_fmaf(a, b, acc);
    } else {
        return acc + b;  // A == 1: identical to fma(1, b, acc)
    }
}

// ----------------------------------------------------------------------------- 16-bit operands (HalfSpmmArgs: spmm_stream.h, spmm_x16.hip)
//
// A 32-bit word of B or C holds two elements, the lower-addressed one in its low half. The kernels carry words in `float` registers
// (loads, stores and moves keep every bit pattern); these helpers are the only places that look inside.
// widen: exact — every fp16 / bf16 value (subnormals included) is an fp32 value.
// narrow: ONE rounding to nearest even; overflow gives +-inf, results that are subnormal in the 16-bit type are rounded, NaN stays NaN.
// bf16 narrows in integer arithmetic, (u + 0x7fff + ((u >> 16) & 1)) >> 16 on the fp32 bits u: the contract of gespmm.h as written.

template <int DT>
__device__ __forceinline__ void widen_x16(float word, float& lo, float& hi) {
    const uint32_t u = __float_as_uint(word);
    if constexpr (DT == kX16Bf16) {
        lo = __uint_as_float(u << 16);
        hi = __uint_as_float(u & 0xffff0000u);
    } else {
        lo = (float)__builtin_bit_cast(_Float16, (uint16_t)(u & 0xffffu));
        hi = (float)__builtin_bit_cast(_Float16, (uint16_t)(u >> 16));
    }
}

template <int DT>
__device__ __forceinline__ uint32_t narrow_x16(float f) {
    if constexpr (DT == kX16Bf16) {
        const uint32_t u = __float_as_uint(f);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;  // NaN: keep it one (quiet bit), whatever the low half held
        return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
    } else {
        return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)f);
    }
}

template <int DT, bool VALUED, int V>
__device__ __forceinline__ void accumulate_x16(float (&acc)[2 * V], float a, const float (&words)[V]) {
#pragma unroll
    for (int i = 0; i < V; ++i) {
        float lo, hi;
        widen_x16<DT>(words[i], lo, hi);
        acc[2 * i] = combine<kReduceSum, VALUED>(acc[2 * i], a, lo);
        acc[2 * i + 1] = combine<kReduceSum, VALUED>(acc[2 * i + 1], a, hi);
    }
}

template <int DT, int V>
__device__ __forceinline__ void pack_x16(float (&words)[V], const float (&acc)[2 * V]) {
#pragma unroll
    for (int i = 0; i < V; ++i) words[i] = __uint_as_float(narrow_x16<DT>(acc[2 * i]) | (narrow_x16<DT>(acc[2 * i + 1]) << 16));
}

}  // namespace gespmm
