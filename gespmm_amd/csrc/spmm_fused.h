// spmm_fused.h — launch table of the FUSED forms of the two streaming kernels (spmm_stream.h with ARGS = FusedSpmmArgs), shared by
// spmm_fused.hip (storage order) and spmm_fused_plan.hip (a plan's task tables).
//
// The library pays for its size when it is loaded, so the fused forms exist for the sum reducer and 32-bit offsets only, and only
// in the lane geometries select.cpp resolves to without launch knobs:
//   batch-stream       V = 1: W = 4 .. 64 (N <= 64) · V = 4: W = 32, 64 and two strips at W = 64 · the narrower vectors of operands
//                      that are not 16-byte aligned: V = 2 at W = 64 (one or two strips), V = 1 with two strips at W = 64
//                      plans only: V = 4 at W = 4, 8, 16 (plan_policy.cpp: narrow_vec4)
//   segmented-stream   V = 1, 4 at W = 32, 64 · V = 4 with two strips · V = 2 at W = 64
//                      plans only: V = 1 at W = 4, 8, 16 (plan_policy.cpp: prefer_segmented at N <= 32)
// Everything else — 64-bit offsets, explicit launch configurations, the max reducer — is the composition route (capi.cpp).
#pragma once
#include "spmm_stream.h"

namespace gespmm {

inline bool fused_geometry_served_impl(const Geometry& g, bool segmented, bool planned) {
    if (g.idx64 || g.reduce != kReduceSum || g.slab_blocked || g.split_long_rows) return false;
    const int V = g.vec, S = g.strips, W = g.group;
    if (W != 4 && W != 8 && W != 16 && W != 32 && W != 64) return false;
    const bool narrow = W < 32;
    if (S == 2) return W == 64 && (V == 4 || (!segmented && (V == 1 || V == 2)));
    if (S != 1) return false;
    if (V == 1) return !narrow || !segmented || planned;
    if (V == 2) return W == 64;
    if (V == 4) return !narrow || (!segmented && planned);
    return false;
}

template <bool VALUED, bool PLANNED>
static hipError_t launch_fused_geometry(const FusedSpmmArgs& a, const Geometry& g, bool segmented, hipStream_t st) {
#define GESPMM_FUSED_STREAM(V_, S_, W_)                           \
    if (!segmented && g.vec == V_ && g.strips == S_ && g.group == W_) \
        return launch_stream<V_, S_, W_, VALUED, false, kReduceSum, PLANNED>(a, g.rows_per_wave, st);
#define GESPMM_FUSED_SEG(V_, S_, W_)                             \
    if (segmented && g.vec == V_ && g.strips == S_ && g.group == W_) \
        return launch_segstream<V_, S_, W_, VALUED, false, kReduceSum, PLANNED>(a, g.rows_per_group, st);
    GESPMM_FUSED_STREAM(1, 1, 4)
    GESPMM_FUSED_STREAM(1, 1, 8)
    GESPMM_FUSED_STREAM(1, 1, 16)
    GESPMM_FUSED_STREAM(1, 1, 32)
    GESPMM_FUSED_STREAM(1, 1, 64)
    GESPMM_FUSED_STREAM(4, 1, 32)
    GESPMM_FUSED_STREAM(4, 1, 64)
    GESPMM_FUSED_STREAM(4, 2, 64)
    GESPMM_FUSED_STREAM(2, 1, 64)
    GESPMM_FUSED_STREAM(2, 2, 64)
    GESPMM_FUSED_STREAM(1, 2, 64)
    GESPMM_FUSED_SEG(1, 1, 32)
    GESPMM_FUSED_SEG(1, 1, 64)
    GESPMM_FUSED_SEG(4, 1, 32)
    GESPMM_FUSED_SEG(4, 1, 64)
    GESPMM_FUSED_SEG(4, 2, 64)
    GESPMM_FUSED_SEG(2, 1, 64)
    if constexpr (PLANNED) {
        GESPMM_FUSED_STREAM(4, 1, 4)
        GESPMM_FUSED_STREAM(4, 1, 8)
        GESPMM_FUSED_STREAM(4, 1, 16)
        GESPMM_FUSED_SEG(1, 1, 4)
        GESPMM_FUSED_SEG(1, 1, 8)
        GESPMM_FUSED_SEG(1, 1, 16)
    }
#undef GESPMM_FUSED_STREAM
#undef GESPMM_FUSED_SEG
    return hipErrorInvalidValue;
}

template <bool PLANNED>
static hipError_t launch_spmm_fused_impl(const FusedSpmmArgs& a, const Geometry& g, bool segmented, hipStream_t st) {
    if (!fused_geometry_served_impl(g, segmented, PLANNED)) return hipErrorInvalidValue;
    return a.val != nullptr ? launch_fused_geometry<true, PLANNED>(a, g, segmented, st)
                            : launch_fused_geometry<false, PLANNED>(a, g, segmented, st);
}

}  // namespace gespmm
