// spmm_heads.h — internal interface of the MULTI-HEAD product (gespmm_csr_spmm_heads_f32; kernels: spmm_heads.hip).
//
// One weight per edge AND head: val is row-major [nnz, H], B is [K, H F], C is [M, H F], and
//   C[r, h F + f] = sum over the entries p of row r, ascending, of fmaf(val[p H + h], B[colind[p] N + h F + f], acc),  N = H F
// — per head the strict-order valued product, one fp32 chain per output element, never a long-row pass.
//
// The kernel is the batch-stream kernel of spmm_stream.h at width N with H weights staged per CSR entry; H is a RUNTIME value under the
// compile-time bound kHeadsMax (the LDS tile is sized for it), so the kernels are one per lane geometry, not one per (geometry, H).
// They exist for 32-bit offsets and the batch-stream geometries select.cpp reaches without launch knobs (the batch-stream list of
// spmm_fused.h):
//   V = 1: W = 4 .. 64 · V = 4: W = 32, 64 and two strips at W = 64 · V = 2 at W = 64 (one or two strips) · V = 1 with two strips at W = 64
//   plans only: V = 4 at W = 4, 8, 16 (plan_policy.cpp: narrow_vec4)
// Everything else — H = 1, H > kHeadsMax, 64-bit offsets — is the composition route (capi.cpp: per head gather, strict product, scatter).
//
// 16-bit B and C (gespmm_csr_spmm_heads_x16; kernels: spmm_heads_x16.hip): the same kernel body (spmm_heads_kernel.h) in 32-bit WORDS —
// HeadsArgs then carries B and C as arrays of words, N = H F / 2 and F = the words of a head, F / 2 — for the storage-order geometries
// above at the width in words. Odd F, operands that are only 2-byte aligned and everything the fp32 kernel leaves to its composition go
// through widen, gespmm_csr_spmm_heads_f32, narrow (capi.cpp): the same bits.
#pragma once
#include "spmm_kernels.h"

namespace gespmm {

constexpr int kHeadsMax = 8;  // heads the kernel serves (2 .. kHeadsMax): 64 x kHeadsMax staged weights per wavefront, 8 KB per workgroup

// val: [nnz, H] (plan mode: in the plan's entry order). V of the launch geometry divides F, so a lane's vector never spans two heads.
struct HeadsArgs : SpmmArgs {
    int32_t H;
    int32_t F;
};

// ... through an edge order (spmm_heads_order.hip): the weights of CSR entry p are row order[p] of val. order: int32[nnz], entries in [0, nnz).
struct HeadsOrderArgs : HeadsArgs {
    const int32_t* order;
};
template <bool ORDERED>
struct HeadsArgsFor {
    using type = HeadsArgs;
};
template <>
struct HeadsArgsFor<true> {
    using type = HeadsOrderArgs;
};
template <bool ORDERED>
using HeadsArgsOf = typename HeadsArgsFor<ORDERED>::type;

inline bool heads_geometry_served(const Geometry& g, bool planned) {
    if (g.idx64 || g.reduce != kReduceSum || g.slab_blocked || g.split_long_rows) return false;
    const int V = g.vec, S = g.strips, W = g.group;
    if (W != 4 && W != 8 && W != 16 && W != 32 && W != 64) return false;
    if (S == 2) return W == 64 && (V == 1 || V == 2 || V == 4);
    if (S != 1) return false;
    if (V == 1) return true;
    if (V == 2) return W == 64;
    if (V == 4) return W >= 32 || planned;
    return false;
}

// a.tasks + a.perm set: the plan-mode kernels. hipErrorInvalidValue where the geometry is not served or H is outside 2 .. kHeadsMax.
hipError_t launch_spmm_heads(const HeadsArgs& a, const Geometry& geo, hipStream_t st);
// spmm_heads_x16.hip: `a` in words (above), storage order only (a.tasks == NULL); hipErrorInvalidValue where the geometry is not served.
hipError_t launch_spmm_heads_x16(const HeadsArgs& a, int dtype, const Geometry& geo, hipStream_t st);
// spmm_heads_order.hip: the storage-order kernels with the weights read through `order` (ORDERED of spmm_heads_kernel.h). dtype 0: `a` as
// launch_spmm_heads takes it; kX16F16 / kX16Bf16: `a` in words as launch_spmm_heads_x16 takes it. a.tasks must be NULL, order not.
hipError_t launch_spmm_heads_order(const HeadsArgs& a, const int32_t* order, int dtype, const Geometry& geo, hipStream_t st);
// ... and out[i, :] = x[order[i], :] for i < n on rows of row_bytes bytes (a multiple of 4; the C entry takes at most 64), order int32 or int64: one
// grid-stride kernel, consecutive lanes on consecutive words of out (16-byte pieces where row_bytes and both arrays allow). An index
// outside [0, n) reads nothing: that row of out is all-ones words.
hipError_t launch_edge_gather(const void* x, const void* order, bool order_is_64, void* out, int64_t n, int64_t row_bytes, hipStream_t st);
// ... and dst[r, 0:width] = src[r, off:off+width] on 16-bit elements (the per-head route of the 16-bit multi-head SDDMM)
hipError_t launch_heads_slice_x16(const void* src, void* dst, int64_t rows, int64_t stride, int64_t off, int64_t width, hipStream_t st);
// The composition route's two copies: dst[r, 0:width] = src[r, off:off+width] (src rows `stride` floats apart) and its inverse
// dst[r, off:off+width] = src[r, 0:width].
hipError_t launch_heads_slice(const float* src, float* dst, int64_t rows, int64_t stride, int64_t off, int64_t width, hipStream_t st);
hipError_t launch_heads_unslice(const float* src, float* dst, int64_t rows, int64_t stride, int64_t off, int64_t width, hipStream_t st);
// val_p[p, :] = val[src_begin[r] + (p - rowptr_p[r]), :] for entry p of row r of a plan's permuted copy: the [nnz, H] weights in the
// plan's entry order (plan.cpp: permute_values, H floats per entry). order (may be NULL): the caller's weights are read through it,
// val_p[p, :] = val[order[src(p)], :] — the two permutations composed in the one copy.
hipError_t launch_permute_head_values(const int32_t* rowptr_p, const int32_t* src_begin, const float* val, float* val_p, int64_t M,
                                      int64_t nnz, int64_t H, hipStream_t st, const int32_t* order = nullptr);

}  // namespace gespmm
