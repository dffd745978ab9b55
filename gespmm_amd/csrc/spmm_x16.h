// spmm_x16.h — launch table of the 16-BIT forms of the two streaming kernels (spmm_stream.h with ARGS = HalfSpmmArgs<DT>), shared by
// spmm_x16.hip (storage order) and spmm_x16_plan.hip (a plan's task tables).
//
// The kernels work in 32-bit words (two elements each), so a geometry here is the fp32 geometry select.cpp resolves for HALF the
// width: V words per lane and strip (2 V elements), W lanes per row. As for the fused forms (spmm_fused.h) the library pays for its
// size when it is loaded: sum reducer and 32-bit offsets only, no launch knobs (gather depth 8, or 4 where V S = 8), and only the lane
// geometries the selector reaches on its own — the same list as spmm_fused.h:
//   batch-stream       V = 1: W = 4 .. 64 (N <= 128) · V = 4: W = 32, 64 and two strips at W = 64 · the narrower vectors of operands
//                      that are not 16-byte aligned or of widths that are no multiple of 8: V = 2 at W = 64 (one or two strips),
//                      V = 1 with two strips at W = 64
//                      plans only: V = 4 at W = 4, 8, 16 (plan_policy.cpp: narrow_vec4)
//   segmented-stream   V = 1, 4 at W = 32, 64 · V = 4 with two strips · V = 2 at W = 64
//                      plans only: V = 1 at W = 4, 8, 16 (plan_policy.cpp: prefer_segmented at narrow widths)
// each for fp16 and bf16, valued and unweighted. Everything else — odd N, operands that are only 2-byte aligned, 64-bit offsets, the
// long-row pass, cache blocking, a plan's table kernels — is the composition route (capi.cpp: widen, the fp32 route, narrow).
#pragma once
#include "spmm_stream.h"

namespace gespmm {

inline bool x16_geometry_served_impl(const Geometry& g, bool segmented, bool planned) {
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

template <int DT, bool VALUED, bool PLANNED>
static hipError_t launch_x16_geometry(const HalfSpmmArgs<DT>& a, const Geometry& g, bool segmented, hipStream_t st) {
#define GESPMM_X16_STREAM(V_, S_, W_)                                 \
    if (!segmented && g.vec == V_ && g.strips == S_ && g.group == W_) \
        return launch_stream<V_, S_, W_, VALUED, false, kReduceSum, PLANNED>(a, g.rows_per_wave, st);
#define GESPMM_X16_SEG(V_, S_, W_)                                   \
    if (segmented && g.vec == V_ && g.strips == S_ && g.group == W_) \
        return launch_segstream<V_, S_, W_, VALUED, false, kReduceSum, PLANNED>(a, g.rows_per_group, st);
    GESPMM_X16_STREAM(1, 1, 4)
    GESPMM_X16_STREAM(1, 1, 8)
    GESPMM_X16_STREAM(1, 1, 16)
    GESPMM_X16_STREAM(1, 1, 32)
    GESPMM_X16_STREAM(1, 1, 64)
    GESPMM_X16_STREAM(4, 1, 32)
    GESPMM_X16_STREAM(4, 1, 64)
    GESPMM_X16_STREAM(4, 2, 64)
    GESPMM_X16_STREAM(2, 1, 64)
    GESPMM_X16_STREAM(2, 2, 64)
    GESPMM_X16_STREAM(1, 2, 64)
    GESPMM_X16_SEG(1, 1, 32)
    GESPMM_X16_SEG(1, 1, 64)
    GESPMM_X16_SEG(4, 1, 32)
    GESPMM_X16_SEG(4, 1, 64)
    GESPMM_X16_SEG(4, 2, 64)
    GESPMM_X16_SEG(2, 1, 64)
    if constexpr (PLANNED) {
        GESPMM_X16_STREAM(4, 1, 4)
        GESPMM_X16_STREAM(4, 1, 8)
        GESPMM_X16_STREAM(4, 1, 16)
        GESPMM_X16_SEG(1, 1, 4)
        GESPMM_X16_SEG(1, 1, 8)
        GESPMM_X16_SEG(1, 1, 16)
    }
#undef GESPMM_X16_STREAM
#undef GESPMM_X16_SEG
    return hipErrorInvalidValue;
}

template <int DT, bool PLANNED>
static hipError_t launch_spmm_x16_dt(const SpmmArgs& words, const Geometry& g, bool segmented, hipStream_t st) {
    HalfSpmmArgs<DT> a;
    static_cast<SpmmArgs&>(a) = words;
    return a.val != nullptr ? launch_x16_geometry<DT, true, PLANNED>(a, g, segmented, st)
                            : launch_x16_geometry<DT, false, PLANNED>(a, g, segmented, st);
}

template <bool PLANNED>
static hipError_t launch_spmm_x16_impl(const SpmmArgs& words, int dtype, const Geometry& g, bool segmented, hipStream_t st) {
    if (!x16_geometry_served_impl(g, segmented, PLANNED)) return hipErrorInvalidValue;
    if (dtype == kX16F16) return launch_spmm_x16_dt<kX16F16, PLANNED>(words, g, segmented, st);
    if (dtype == kX16Bf16) return launch_spmm_x16_dt<kX16Bf16, PLANNED>(words, g, segmented, st);
    return hipErrorInvalidValue;
}

}  // namespace gespmm
