// capi.cpp — the extern "C" boundary declared in include/gespmm.h.
//
// Argument validation, variant -> launch-geometry selection, and the hand-off to
// the HIP launchers. Nothing here touches device memory; the only HIP calls are
// the kernel launches themselves. There is deliberately no CPU fallback: on a
// machine without a HIP device the launch fails and its hipError_t is returned.

#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/gespmm.h"
#include "select.h"
#include "auto_plan.h"
#include "edge_softmax.h"
#include "plan.h"
#include "sddmm_heads.h"
#include "spmm_heads.h"
#include "spmm_kernels.h"
#include "workspace.h"

namespace {

using gespmm::Geometry;
using gespmm::SpmmArgs;

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

int check_common(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B, const float* C,
                 int64_t M, int64_t K, int64_t N, int64_t nnz) {
    if (M < 0 || K < 0 || N < 0 || nnz < -1) return GESPMM_EINVAL;
    // CSR positions are int32 and the kernels look up to a few tiles past a row's end before clamping
    if (M > 0x7fffffffLL - 64 || K > 0x7fffffffLL || N > 0x7fffffffLL / 4 || nnz > 0x7fffffffLL - 4096)
        return GESPMM_ERANGE;
    if (M == 0 || N == 0) return 0;  // nothing to do; pointers may be null
    if (!rowptr || !C) return GESPMM_EINVAL;
    if ((nnz != 0) && (!colind || !B)) return GESPMM_EINVAL;
    if (!aligned_to(rowptr, 4) || !aligned_to(colind, 4) || !aligned_to(val, 4) || !aligned_to(B, 4) ||
        !aligned_to(C, 4))
        return GESPMM_EALIGN;
    return 0;
}

}  // namespace

namespace gespmm {

// The one place every SpMM entry point ends up in (plan.cpp included: `pl` carries the plan's task table).
int run_spmm(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B, float* C, int64_t M,
             int64_t K, int64_t N, int64_t nnz, int variant, const gespmm_launch_cfg* cfg, int reduce, float empty,
             void* stream, void* ws, int64_t ws_bytes, const PlanLaunch* pl, const LaunchGuard* guard) {
    const int rc = check_common(rowptr, colind, val, B, C, M, K, N, nnz);
    if (rc != 0) return rc;
    if (M == 0 || N == 0) return 0;
    if (variant < GESPMM_VARIANT_AUTO || variant >= GESPMM_NUM_VARIANTS) return GESPMM_EINVAL;
    if (reduce == gespmm::kReduceMax && (val != nullptr || variant == GESPMM_VARIANT_PARREDUCE ||
                                         variant == GESPMM_VARIANT_NAIVE))
        return GESPMM_EINVAL;
    if (cfg && (cfg->rows_per_wave < 0 || cfg->rows_per_wave > gespmm::kMaxRowsPerWave || cfg->slab_rows < 0))
        return GESPMM_EINVAL;

    // Vector width is limited by what both B and C rows can be addressed with.
    int max_vec = 4;
    while (max_vec > 1 && ((N % max_vec) != 0 || !aligned_to(B, 4u * max_vec) || !aligned_to(C, 4u * max_vec)))
        max_vec >>= 1;

    gespmm::Selection sel;
    int flags = 0;
    if (cfg) flags = cfg->flags;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    {
        // Under stream capture the paths that need a stream-ordered temporary are switched off: a
        // captured allocation becomes a mem-alloc graph node, and replaying those costs seconds per
        // launch on this runtime (measured: 14 s per GCN epoch on reddit-like instead of 20 ms).
        // The streaming kernels need no workspace and give the same bits (slab path) or the strict
        // CSR-order chain (long-row pass).
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (ws != nullptr && ws_bytes > 0) {
            // the caller's workspace: nothing is allocated whether capturing or not (a workspace that
            // turns out too small falls back to the pool — gespmm_csr_spmm_workspace_bytes is an upper bound)
        } else if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
            flags |= gespmm::kFlagNoSlabBlocked | gespmm::kFlagStrictOrder;
            flags &= ~(gespmm::kFlagSlabBlocked | gespmm::kFlagSplitLongRows);
        } else {
            (void)hipGetLastError();
        }
    }
    if (pl) {  // task tables exist for the two streaming kernels only
        flags |= gespmm::kFlagNoSlabBlocked;
        flags &= ~(gespmm::kFlagSlabBlocked | gespmm::kFlagSegStream | gespmm::kFlagBatchStream);
        flags |= (pl->prefer_segmented && pl->gtasks) ? gespmm::kFlagSegStream : gespmm::kFlagBatchStream;
        flags &= ~gespmm::kFlagAllowReassoc;  // a plan runs the CRC family only (the parallel-reduction variant has no task table)
    }
    const int src = gespmm::resolve_geometry(M, K, N, nnz, variant, max_vec, cfg ? cfg->vec : 0,
                                             cfg ? cfg->strips : 0, cfg ? cfg->group : 0,
                                             cfg ? cfg->rows_per_wave : 0, cfg ? cfg->slab_rows : 0, flags, &sel);
    if (src != 0) return src;
    sel.geo.reduce = reduce;
    if (pl && (sel.variant == GESPMM_VARIANT_NAIVE || sel.variant == GESPMM_VARIANT_PARREDUCE)) return GESPMM_EINVAL;

    SpmmArgs a;
    a.rowptr = rowptr;
    a.colind = colind;
    a.val = val;
    a.B = B;
    a.C = C;
    a.M = (int32_t)M;
    a.N = (int32_t)N;
    a.nblk = 0;
    a.ntile = 0;
    a.flags = flags | (sel.geo.sc1_store ? gespmm::kFlagSc1Store : 0);
    a.empty = empty;
    a.long_row = 0;
    a.lr_hdr = nullptr;
    a.lr_rows = nullptr;
    a.lr_chunks = nullptr;
    a.lr_chunk = a.lr_max_rows = a.lr_max_chunks = 0;
    a.row_begin = nullptr;
    a.row_end = nullptr;
    a.accumulate = 0;
    a.tasks = pl ? pl->tasks : nullptr;
    a.perm = pl ? pl->perm : nullptr;
    a.ntasks = pl ? pl->ntasks : 0;
    a.gtasks = pl ? pl->gtasks : nullptr;
    a.ngtasks = pl ? pl->ngtasks : 0;
    a.guard = guard ? guard->word : nullptr;
    a.guard_want = guard ? guard->want : 0;
    // a guard covers ONE kernel: the two streaming kernels without the long-row pass
    if (guard && (sel.variant == GESPMM_VARIANT_PARREDUCE || sel.variant == GESPMM_VARIANT_NAIVE || sel.geo.slab_blocked ||
                  sel.geo.split_long_rows))
        return gespmm::kNotGuardable;
    if (guard && guard->word == nullptr) return 0;  // dry run (auto_plan.cpp): would this call be one guardable kernel? nothing is launched

    hipError_t e;
    a.rpw = sel.geo.rows_per_group;
    if (sel.variant == GESPMM_VARIANT_PARREDUCE) e = gespmm::launch_spmm_parreduce(a, sel.geo, st);
    else if (sel.variant == GESPMM_VARIANT_NAIVE)
        e = gespmm::launch_spmm_naive(a, sel.geo, st);
    else if (sel.geo.slab_blocked) {
        // rows per lane group and launch: 2 measured best on reddit-like at N = 64..256 (hub rows make
        // 8-row tasks a long tail: 45 % average occupancy in the PMC run), profiles/r01/slab_task_size.log
        a.rpw = (cfg && cfg->rows_per_wave > 0) ? cfg->rows_per_wave : 2;
        e = gespmm::launch_spmm_slabblocked(a, sel.geo, ws, (size_t)(ws_bytes > 0 ? ws_bytes : 0), st);
    } else {
        bool seg = sel.geo.segmented;
        if (flags & gespmm::kFlagBatchStream) seg = false;
        if ((flags & gespmm::kFlagSegStream) && !sel.geo.split_long_rows) seg = true;
        // operands that are only 4- or 8-byte aligned resolve to a narrower vector; two strips of < 4 floats have no
        // segmented-stream instantiation: a plan then runs its wavefront task table (any N and alignment stay legal)
        if (seg && pl && sel.geo.strips == 2 && sel.geo.vec < 4) seg = false;
        if (seg) e = gespmm::launch_spmm_segstream(a, sel.geo, st);
        else {
            a.rpw = sel.geo.rows_per_wave;
            a.long_row = sel.geo.split_long_rows ? sel.geo.long_row_threshold : 0;
            if (sel.geo.split_long_rows)
                e = gespmm::launch_spmm_stream_with_longrows(a, sel.geo, nnz, ws, (size_t)(ws_bytes > 0 ? ws_bytes : 0), st);
            else
                e = gespmm::launch_spmm_stream(a, sel.geo, st);
        }
    }
    return (int)e;
}

int check_fused_args(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B, const FusedVectors& fx, const float* C,
                     int64_t M, int64_t K, int64_t N, int64_t nnz) {
    const int rc = check_common(rowptr, colind, val, B, C, M, K, N, nnz);
    if (rc != 0) return rc;
    if (!aligned_to(fx.col_scale, 4) || !aligned_to(fx.row_scale, 4) || !aligned_to(fx.bias, 4)) return GESPMM_EALIGN;
    return 0;
}

int refuse_allocation_under_capture(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return (int)hipErrorStreamCaptureUnsupported;
    (void)hipGetLastError();
    return 0;
}

// The fused counterpart of run_spmm: the same selection (a plan's task tables included), then ONE fused streaming kernel or nothing.
int run_spmm_fused(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B, const FusedVectors& fx, float* C,
                   int64_t M, int64_t K, int64_t N, int64_t nnz, int variant, int flags, void* stream, const PlanLaunch* pl, bool dry_run,
                   int* kind) {
    *kind = 0;
    if (variant < GESPMM_VARIANT_AUTO || variant >= GESPMM_NUM_VARIANTS) return GESPMM_EINVAL;
    if (M <= 0 || N <= 0) return kFusedUnavailable;
    // Vector width: what B, C and the bias slice can be addressed with (the bits do not depend on it).
    int max_vec = 4;
    while (max_vec > 1 && ((N % max_vec) != 0 || (!dry_run && (!aligned_to(B, 4u * max_vec) || !aligned_to(C, 4u * max_vec) ||
                                                               !aligned_to(fx.bias, 4u * max_vec)))))
        max_vec >>= 1;
    if (pl) {  // (as run_spmm: task tables exist for the two streaming kernels only)
        flags |= kFlagNoSlabBlocked;
        flags &= ~(kFlagSlabBlocked | kFlagSegStream | kFlagBatchStream);
        flags |= (pl->prefer_segmented && pl->gtasks) ? kFlagSegStream : kFlagBatchStream;
        flags &= ~kFlagAllowReassoc;
    }
    Selection sel;
    if (resolve_geometry(M, K, N, nnz, variant, max_vec, 0, 0, 0, 0, 0, flags, &sel) != 0) return GESPMM_EINVAL;
    sel.geo.reduce = kReduceSum;
    if (sel.variant == GESPMM_VARIANT_NAIVE || sel.variant == GESPMM_VARIANT_PARREDUCE) return kFusedUnavailable;
    bool seg = sel.geo.segmented;
    if (flags & kFlagBatchStream) seg = false;
    if ((flags & kFlagSegStream) && !sel.geo.split_long_rows) seg = true;
    if (seg && pl && sel.geo.strips == 2 && sel.geo.vec < 4) seg = false;
    if (!fused_geometry_served(sel.geo, seg, pl != nullptr)) return kFusedUnavailable;  // (long-row pass, cache blocking, 64-bit offsets too)
    *kind = seg ? 2 : 1;
    if (dry_run) return 0;

    FusedSpmmArgs a = {};
    a.rowptr = rowptr;
    a.colind = colind;
    a.val = val;
    a.B = B;
    a.C = C;
    a.M = (int32_t)M;
    a.N = (int32_t)N;
    a.flags = flags;
    a.rpw = seg ? sel.geo.rows_per_group : sel.geo.rows_per_wave;
    a.tasks = pl ? pl->tasks : nullptr;
    a.perm = pl ? pl->perm : nullptr;
    a.ntasks = pl ? pl->ntasks : 0;
    a.gtasks = pl ? pl->gtasks : nullptr;
    a.ngtasks = pl ? pl->ngtasks : 0;
    a.col_scale = fx.col_scale;
    a.row_scale = fx.row_scale;
    a.bias = fx.bias;
    return (int)launch_spmm_fused(a, sel.geo, seg, reinterpret_cast<hipStream_t>(stream));
}

// ---- 16-bit dense operands (gespmm.h: gespmm_csr_spmm_x16). The argument checks of both entry points, no device work.
int check_x16_args(const int32_t* rowptr, const int32_t* colind, const float* val, const void* B, const void* C, int dtype, int64_t M,
                   int64_t K, int64_t N, int64_t nnz) {
    if (dtype != GESPMM_X16_F16 && dtype != GESPMM_X16_BF16) return GESPMM_EINVAL;
    if (M < 0 || K < 0 || N < 0 || nnz < -1) return GESPMM_EINVAL;
    if (M > 0x7fffffffLL - 64 || K > 0x7fffffffLL || N > 0x7fffffffLL / 4 || nnz > 0x7fffffffLL - 4096) return GESPMM_ERANGE;
    if (M == 0 || N == 0) return 0;
    if (!rowptr || !C) return GESPMM_EINVAL;
    if ((nnz != 0) && (!colind || !B)) return GESPMM_EINVAL;
    if (!aligned_to(rowptr, 4) || !aligned_to(colind, 4) || !aligned_to(val, 4) || !aligned_to(B, 2) || !aligned_to(C, 2)) return GESPMM_EALIGN;
    return 0;
}

int pointer_alignment(const void* p) {  // largest power of two (<= 16) that divides the address
    int a = 16;
    while (a > 1 && reinterpret_cast<uintptr_t>(p) % (uintptr_t)a != 0) a >>= 1;
    return a;
}

// The 16-bit counterpart of run_spmm_fused: ONE 16-bit streaming kernel or nothing (kX16Unavailable: the caller composes widen, the fp32
// route, narrow). The kernels work in 32-bit words, so the geometry is the one the selector resolves for the byte-equivalent fp32 width
// N / 2 — every rule of select.cpp is about bytes and lanes per row — with V limited by what B and C can be addressed with, in words.
// b_align / c_align: powers of two dividing the operands' addresses (>= 16 is as good as 16); dry_run: the answer only.
int run_spmm_x16(const int32_t* rowptr, const int32_t* colind, const float* val, const void* B, void* C, int dtype, int64_t M, int64_t K,
                 int64_t N, int64_t nnz, int variant, int flags, void* stream, const PlanLaunch* pl, int b_align, int c_align, bool dry_run,
                 int* kind, Geometry* geo_out) {
    *kind = 0;
    if (variant < GESPMM_VARIANT_AUTO || variant >= GESPMM_NUM_VARIANTS) return GESPMM_EINVAL;
    if (M <= 0 || N <= 0 || N % 2 != 0 || b_align < 4 || c_align < 4) return kX16Unavailable;
    const int64_t Nw = N / 2;  // words per row
    int max_vec = 4;
    while (max_vec > 1 && ((Nw % max_vec) != 0 || b_align < 4 * max_vec || c_align < 4 * max_vec)) max_vec >>= 1;
    if (!dry_run) {  // (as run_spmm: a capturing stream takes the streaming kernels, which allocate nothing)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(reinterpret_cast<hipStream_t>(stream), &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
            flags |= kFlagNoSlabBlocked | kFlagStrictOrder;
            flags &= ~(kFlagSlabBlocked | kFlagSplitLongRows);
        } else {
            (void)hipGetLastError();
        }
    }
    if (pl) {  // (as run_spmm: task tables exist for the two streaming kernels only)
        flags |= kFlagNoSlabBlocked;
        flags &= ~(kFlagSlabBlocked | kFlagSegStream | kFlagBatchStream);
        flags |= (pl->prefer_segmented && pl->gtasks) ? kFlagSegStream : kFlagBatchStream;
        flags &= ~kFlagAllowReassoc;
    }
    Selection sel;
    if (resolve_geometry(M, K, Nw, nnz, variant, max_vec, 0, 0, 0, 0, 0, flags, &sel) != 0) return GESPMM_EINVAL;
    sel.geo.reduce = kReduceSum;
    if (sel.variant == GESPMM_VARIANT_NAIVE || sel.variant == GESPMM_VARIANT_PARREDUCE) return kX16Unavailable;
    bool seg = sel.geo.segmented;
    if (flags & kFlagBatchStream) seg = false;
    if ((flags & kFlagSegStream) && !sel.geo.split_long_rows) seg = true;
    if (seg && pl && sel.geo.strips == 2 && sel.geo.vec < 4) seg = false;
    if (!x16_geometry_served(sel.geo, seg, pl != nullptr)) return kX16Unavailable;  // (long-row pass, cache blocking, 64-bit offsets too)
    *kind = seg ? 2 : 1;
    if (geo_out) *geo_out = sel.geo;
    if (dry_run) return 0;

    SpmmArgs a = {};
    a.rowptr = rowptr;
    a.colind = colind;
    a.val = val;
    a.B = static_cast<const float*>(B);  // (arrays of words: spmm_kernels.h, HalfSpmmArgs)
    a.C = static_cast<float*>(C);
    a.M = (int32_t)M;
    a.N = (int32_t)Nw;
    a.flags = flags;
    a.rpw = seg ? sel.geo.rows_per_group : sel.geo.rows_per_wave;
    a.tasks = pl ? pl->tasks : nullptr;
    a.perm = pl ? pl->perm : nullptr;
    a.ntasks = pl ? pl->ntasks : 0;
    a.gtasks = pl ? pl->gtasks : nullptr;
    a.ngtasks = pl ? pl->ngtasks : 0;
    return (int)launch_spmm_x16(a, dtype, sel.geo, seg, reinterpret_cast<hipStream_t>(stream));
}

// ---- the multi-head product (gespmm.h: gespmm_csr_spmm_heads_f32). The argument checks of both entry points, no device work.
int check_heads_sizes(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz) {
    if (H < 1 || M < 0 || K < 0 || F < 0 || nnz < 0) return GESPMM_EINVAL;
    if (M > 0x7fffffffLL - 64 || K > 0x7fffffffLL || H > 0x7fffffffLL / 4 || F > (0x7fffffffLL / 4) / H || nnz > 0x7fffffffLL - 4096)
        return GESPMM_ERANGE;  // (H F, the width, within what the other entries take as N)
    return 0;
}

int check_heads_args(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B, const float* C, int64_t M, int64_t K,
                     int64_t H, int64_t F, int64_t nnz) {
    const int rc = check_heads_sizes(M, K, H, F, nnz);
    if (rc != 0) return rc;
    if (M == 0 || F == 0) return 0;
    if (!rowptr || !C) return GESPMM_EINVAL;
    if ((nnz != 0) && (!colind || !B || !val)) return GESPMM_EINVAL;
    if (!aligned_to(rowptr, 4) || !aligned_to(colind, 4) || !aligned_to(val, 4) || !aligned_to(B, 4) || !aligned_to(C, 4)) return GESPMM_EALIGN;
    return 0;
}

// The multi-head counterpart of run_spmm_x16: ONE heads kernel or nothing (kHeadsUnavailable: the caller composes per head). The geometry
// is what the selector resolves for width N = H F with the batch-stream kernel forced, strict order and no cache blocking; V is limited
// to what divides F (a lane's vector stays inside one head) and to what B and C can be addressed with.
int run_spmm_heads(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B, float* C, int64_t M, int64_t K, int64_t H,
                   int64_t F, int64_t nnz, int variant, int flags, void* stream, const PlanLaunch* pl, int b_align, int c_align, bool dry_run,
                   int* kind, Geometry* geo_out) {
    *kind = 0;
    if (variant < GESPMM_VARIANT_AUTO || variant >= GESPMM_NUM_VARIANTS) return GESPMM_EINVAL;
    if (H < 2 || H > kHeadsMax || M <= 0 || F <= 0 || nnz < 0 || b_align < 4 || c_align < 4) return kHeadsUnavailable;
    // GESPMM_HEADS_ROUTE=composition pins route 0 (read per call: scripts/heads_timing.py measures both routes in one process)
    if (const char* env = getenv("GESPMM_HEADS_ROUTE"))
        if (!strcmp(env, "composition")) return kHeadsUnavailable;
    const int64_t N = H * F;
    if ((uint64_t)K * (uint64_t)N * 4ull >= (1ull << 32) || nnz * H >= (1ll << 31)) return kHeadsUnavailable;  // 32-bit offsets only
    int max_vec = 4;
    while (max_vec > 1 && ((F % max_vec) != 0 || b_align < 4 * max_vec || c_align < 4 * max_vec)) max_vec >>= 1;
    flags |= kFlagBatchStream | kFlagStrictOrder | kFlagNoSlabBlocked;
    flags &= ~(kFlagSegStream | kFlagSlabBlocked | kFlagSplitLongRows | kFlagAllowReassoc | kFlagForceIdx64);
    Selection sel;
    if (resolve_geometry(M, K, N, nnz, variant, max_vec, 0, 0, 0, 0, 0, flags, &sel) != 0) return GESPMM_EINVAL;
    sel.geo.reduce = kReduceSum;
    if (sel.variant == GESPMM_VARIANT_NAIVE || sel.variant == GESPMM_VARIANT_PARREDUCE) return kHeadsUnavailable;
    if (!heads_geometry_served(sel.geo, pl != nullptr)) return kHeadsUnavailable;
    *kind = 1;
    if (geo_out) *geo_out = sel.geo;
    if (dry_run) return 0;
    if (nnz != 0 && (!val || !colind || !B)) return GESPMM_EINVAL;  // (no entries: the kernel reads none of the three and writes zeros)

    HeadsArgs a = {};
    a.rowptr = rowptr;
    a.colind = colind;
    a.val = val;
    a.B = B;
    a.C = C;
    a.M = (int32_t)M;
    a.N = (int32_t)N;
    a.flags = flags;
    a.rpw = sel.geo.rows_per_wave;
    a.tasks = pl ? pl->tasks : nullptr;
    a.perm = pl ? pl->perm : nullptr;
    a.ntasks = pl ? pl->ntasks : 0;
    a.H = (int32_t)H;
    a.F = (int32_t)F;
    return (int)launch_spmm_heads(a, sel.geo, reinterpret_cast<hipStream_t>(stream));
}

// ---- the multi-head SDDMM (gespmm.h: gespmm_sddmm_{coo,csr}_heads_f32; sddmm_heads.h). GESPMM_SDDMM_HEADS_ROUTE=kernel|composition pins
// the route (read per call: scripts/sddmm_heads_timing.py measures both in one process); resolve_sddmm_heads says where a pin is ignored.
int sddmm_heads_pin() {
    if (const char* env = getenv("GESPMM_SDDMM_HEADS_ROUTE")) {
        if (!strcmp(env, "kernel")) return kSddmmHeadsPinKernel;
        if (!strcmp(env, "composition")) return kSddmmHeadsPinComposition;
    }
    return kSddmmHeadsPinNone;
}

// ---- the edge softmax (gespmm.h: gespmm_edge_softmax_f32 / _backward_f32; edge_softmax.h). Sizes alone: what makes no sense, then what is
// too large for the kernel's 32-bit word positions p H + h (there is no other route).
int check_edge_softmax_sizes(int64_t M, int64_t H, int64_t nnz, float slope) {
    if (M < 0 || H < 1 || nnz < 0 || !std::isfinite(slope) || (M == 0 && nnz > 0)) return GESPMM_EINVAL;
    if (M > kEdgeSoftmaxMaxRows || H > kSddmmMaxNnz || nnz > kSddmmMaxNnz / H) return GESPMM_ERANGE;
    return 0;
}

// Sizes alone, as check_heads_sizes: csr == false ignores M, and has no composition to take a pair count past the kernel's limit.
int check_sddmm_heads_sizes(bool csr, int64_t M, int64_t H, int64_t F, int64_t nnz) {
    if (H < 1 || F < 0 || nnz < 0 || (csr && M < 0)) return GESPMM_EINVAL;
    if ((csr && M > 0x7fffffffLL - 1) || nnz > kSddmmMaxNnz || H > 0x7fffffffLL / 4 || F > (0x7fffffffLL / 4) / H) return GESPMM_ERANGE;
    if (!csr && nnz > kSddmmMaxNnz / H) return GESPMM_ERANGE;
    return 0;
}

// The checks of gespmm_sddmm_{coo,csr}_f32, in their order. 1: nothing left to do (no edges).
int check_sddmm_heads_args(const int32_t* rows, bool csr, const int32_t* colind, const float* D1, const float* D2, const float* out, int64_t M,
                           int64_t H, int64_t F, int64_t nnz) {
    const int rc = check_sddmm_heads_sizes(csr, M, H, F, nnz);
    if (rc != 0) return rc;
    if (nnz == 0) return 1;
    if (!rows || !colind || !out || (F > 0 && (!D1 || !D2))) return GESPMM_EINVAL;
    if (!aligned_to(rows, 4) || !aligned_to(colind, 4) || !aligned_to(D1, 4) || !aligned_to(D2, 4) || !aligned_to(out, 4)) return GESPMM_EALIGN;
    return 0;
}

// One multi-head SDDMM on checked arguments, nnz > 0: what resolve_sddmm_heads answers, nothing else.
//   plain        H == 1: launch_sddmm on the caller's arrays.
//   kernel       one sddmm_heads_kernel; never allocates.
//   composition  CSR only (past the kernel's pair limit, or pinned). Per head: D1[:, hF:(h+1)F] and D2[:, hF:(h+1)F] into stream-ordered temporaries that start address(D) % 16
//                bytes past a 256-byte boundary — the caller's alignment class, hence the caller's V — launch_sddmm at width F into an
//                nnz temporary, scatter into out[:, h]. K < 0: the call does not say how many rows D2 has; 1 + the largest column index
//                is found on the device and read back (one stream synchronisation; a plan passes its K).
int run_sddmm_heads(const int32_t* rows, bool csr, const int32_t* colind, const float* D1, const float* D2, float* out, int64_t M, int64_t K,
                    int64_t H, int64_t F, int64_t nnz, void* stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (F == 0) return (int)hipMemsetAsync(out, 0, (size_t)nnz * (size_t)H * sizeof(float), st);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
    (void)hipGetLastError();
    const SddmmHeadsLaunch r = resolve_sddmm_heads(csr, M, nnz, H, F, pointer_alignment(D1), pointer_alignment(D2), capturing, sddmm_heads_pin());
    if (r.route == kSddmmHeadsPlain) return (int)launch_sddmm(rows, csr, colind, D1, D2, out, M, nnz, F, st);
    if (r.route == kSddmmHeadsKernel) return (int)launch_sddmm_heads(rows, colind, D1, D2, out, M, nnz, H, F, r, st);
    if (!csr) return GESPMM_ERANGE;  // (check_sddmm_heads_sizes lets no such call through)
    int rc = refuse_allocation_under_capture(st);
    if (rc != 0) return rc;  // (nothing launched)
    if (K < 0) {
        int32_t* d_max = nullptr;
        int32_t h_max = 0;
        hipError_t e = workspace_alloc(reinterpret_cast<void**>(&d_max), 256, st);
        if (e != hipSuccess) return (int)e;
        e = launch_max_index(colind, nnz, d_max, st);
        if (e == hipSuccess) e = hipMemcpyAsync(&h_max, d_max, sizeof h_max, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        const hipError_t ef = workspace_free(d_max, st);
        if (e != hipSuccess || ef != hipSuccess) return (int)(e != hipSuccess ? e : ef);
        K = (int64_t)h_max + 1;
    }
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t d1_bytes = up((size_t)M * (size_t)F * 4 + 16), d2_bytes = up((size_t)K * (size_t)F * 4 + 16), t_bytes = (size_t)nnz * 4;
    char* scratch = nullptr;
    hipError_t e = workspace_alloc(reinterpret_cast<void**>(&scratch), d1_bytes + d2_bytes + t_bytes, st);
    if (e != hipSuccess) return (int)e;
    float* D1h = reinterpret_cast<float*>(scratch + reinterpret_cast<uintptr_t>(D1) % 16);
    float* D2h = reinterpret_cast<float*>(scratch + d1_bytes + reinterpret_cast<uintptr_t>(D2) % 16);
    float* th = reinterpret_cast<float*>(scratch + d1_bytes + d2_bytes);
    const int64_t N = H * F;
    for (int64_t h = 0; h < H && rc == 0; ++h) {  // (stream order keeps one head's temporaries until its scatter has read them)
        rc = (int)launch_heads_slice(D1, D1h, M, N, h * F, F, st);
        if (rc == 0) rc = (int)launch_heads_slice(D2, D2h, K, N, h * F, F, st);
        if (rc == 0) rc = (int)launch_sddmm(rows, true, colind, D1h, D2h, th, M, nnz, F, st);
        if (rc == 0) rc = (int)launch_heads_unslice(th, out, nnz, H, h, 1, st);
    }
    e = workspace_free(scratch, st);
    if (rc == 0) rc = (int)e;
    return rc;
}

}  // namespace gespmm

namespace {
int run_spmm(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B, float* C, int64_t M,
             int64_t K, int64_t N, int64_t nnz, int variant, const gespmm_launch_cfg* cfg, int reduce, float empty,
             void* stream, void* ws = nullptr, int64_t ws_bytes = 0) {
    return gespmm::run_spmm(rowptr, colind, val, B, C, M, K, N, nnz, variant, cfg, reduce, empty, stream, ws, ws_bytes,
                            nullptr);
}
}  // namespace

extern "C" {

const char* gespmm_version(void) {
    static char buf[64];
    if (!buf[0]) snprintf(buf, sizeof buf, "gespmm %d.%d (gfx950)", GESPMM_VERSION_MAJOR, GESPMM_VERSION_MINOR);
    return buf;
}

const char* gespmm_error_string(int code) {
    switch (code) {
        case 0: return "success";
        case GESPMM_EINVAL: return "gespmm: invalid argument";
        case GESPMM_EALIGN: return "gespmm: pointer not 4-byte aligned";
        case GESPMM_ERANGE: return "gespmm: size exceeds int32 CSR addressing";
        case GESPMM_EIO: return "gespmm: file not found or unreadable";
        case GESPMM_EFORMAT: return "gespmm: could not process Matrix Market banner or size line";
        case GESPMM_ENOMEM: return "gespmm: host allocation failed";
    }
    if (code > 0) return hipGetErrorString((hipError_t)code);
    return "gespmm: unknown error code";
}

int gespmm_csr_spmm_f32(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B, float* C,
                        int64_t M, int64_t K, int64_t N, int64_t nnz, int variant, void* stream) {
    if (gespmm::auto_plan_enabled()) {  // (gespmm_set_auto_plan: off by default — one relaxed load)
        int rc = 0;
        if (check_common(rowptr, colind, val, B, C, M, K, N, nnz) == 0 && variant >= GESPMM_VARIANT_AUTO && variant < GESPMM_NUM_VARIANTS &&
            variant != GESPMM_VARIANT_NAIVE && variant != GESPMM_VARIANT_PARREDUCE &&  // (a plan runs the CRC family)
            gespmm::auto_plan_try(rowptr, colind, val, B, C, M, K, N, nnz, variant, gespmm::kReduceSum, 0.0f, stream, &rc))
            return rc;
    }
    return run_spmm(rowptr, colind, val, B, C, M, K, N, nnz, variant, nullptr, gespmm::kReduceSum, 0.0f, stream);
}

// The fused product (gespmm.h): one fused streaming kernel where the unfused call would be one streaming kernel, else the
// composition — prescale into a stream-ordered temporary, the unfused call, the in-place epilogue. Same bits either way.
int gespmm_csr_spmm_fused_f32(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B, const float* col_scale,
                              const float* row_scale, const float* bias, float* C, int64_t M, int64_t K, int64_t N, int64_t nnz,
                              int variant, void* stream) {
    const gespmm::FusedVectors fx = {col_scale, row_scale, bias};
    const int rc0 = gespmm::check_fused_args(rowptr, colind, val, B, fx, C, M, K, N, nnz);
    if (rc0 != 0) return rc0;
    if (variant < GESPMM_VARIANT_AUTO || variant >= GESPMM_NUM_VARIANTS) return GESPMM_EINVAL;
    if (M == 0 || N == 0) return 0;
    if (!fx.any()) return gespmm_csr_spmm_f32(rowptr, colind, val, B, C, M, K, N, nnz, variant, stream);
    int kind = 0;
    int rc = gespmm::run_spmm_fused(rowptr, colind, val, B, fx, C, M, K, N, nnz, variant, 0, stream, nullptr, false, &kind);
    if (rc != gespmm::kFusedUnavailable) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    void* scratch = nullptr;
    const float* Bin = B;
    if (col_scale && K > 0 && nnz != 0) {
        if ((rc = gespmm::refuse_allocation_under_capture(st)) != 0) return rc;
        hipError_t e = gespmm::workspace_alloc(&scratch, (size_t)K * (size_t)N * 4, st);
        if (e == hipSuccess) e = gespmm::launch_scale_rows(B, col_scale, static_cast<float*>(scratch), K, N, st);
        if (e != hipSuccess) {
            if (scratch) (void)gespmm::workspace_free(scratch, st);
            return (int)e;
        }
        Bin = static_cast<const float*>(scratch);
    }
    rc = run_spmm(rowptr, colind, val, Bin, C, M, K, N, nnz, variant, nullptr, gespmm::kReduceSum, 0.0f, stream);
    if (rc == 0) rc = (int)gespmm::launch_scale_bias_inplace(C, row_scale, bias, M, N, st);
    if (scratch) {
        const hipError_t e = gespmm::workspace_free(scratch, st);
        if (rc == 0) rc = (int)e;
    }
    return rc;
}

// 16-bit dense operands (gespmm.h): one 16-bit streaming kernel where the byte-equivalent fp32 call would be one streaming kernel, else
// the composition — widen B into a stream-ordered temporary, the fp32 call unchanged into a second one, narrow into C. Same bits:
// widening is exact and either way the fp32 sum is rounded once.
int gespmm_csr_spmm_x16(const int32_t* rowptr, const int32_t* colind, const float* val, const void* B, void* C, int dtype, int64_t M,
                        int64_t K, int64_t N, int64_t nnz, int variant, void* stream) {
    const int rc0 = gespmm::check_x16_args(rowptr, colind, val, B, C, dtype, M, K, N, nnz);
    if (rc0 != 0) return rc0;
    if (variant < GESPMM_VARIANT_AUTO || variant >= GESPMM_NUM_VARIANTS) return GESPMM_EINVAL;
    if (M == 0 || N == 0) return 0;
    int kind = 0;
    int rc = gespmm::run_spmm_x16(rowptr, colind, val, B, C, dtype, M, K, N, nnz, variant, 0, stream, nullptr, gespmm::pointer_alignment(B),
                                  gespmm::pointer_alignment(C), false, &kind);
    if (rc != gespmm::kX16Unavailable) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if ((rc = gespmm::refuse_allocation_under_capture(st)) != 0) return rc;  // (nothing launched)
    const size_t b_bytes = (((size_t)K * (size_t)N * 4) + 255) & ~(size_t)255, c_bytes = (size_t)M * (size_t)N * 4;
    void* scratch = nullptr;
    hipError_t e = gespmm::workspace_alloc(&scratch, b_bytes + c_bytes, st);
    if (e != hipSuccess) return (int)e;
    float* Bf = static_cast<float*>(scratch);
    float* Cf = reinterpret_cast<float*>(static_cast<char*>(scratch) + b_bytes);
    if (B && nnz != 0) e = gespmm::launch_widen_x16(B, Bf, dtype, K * N, st);
    rc = (int)e;
    if (rc == 0) rc = run_spmm(rowptr, colind, val, Bf, Cf, M, K, N, nnz, variant, nullptr, gespmm::kReduceSum, 0.0f, stream);
    if (rc == 0) rc = (int)gespmm::launch_narrow_x16(Cf, C, dtype, M * N, st);
    e = gespmm::workspace_free(scratch, st);
    if (rc == 0) rc = (int)e;
    return rc;
}

int gespmm_x16_route(int64_t M, int64_t K, int64_t N, int64_t nnz, int variant, int b_align, int c_align) {
    if (M < 0 || K < 0 || N < 0 || nnz < -1 || b_align < 1 || c_align < 1) return GESPMM_EINVAL;
    if (variant < GESPMM_VARIANT_AUTO || variant >= GESPMM_NUM_VARIANTS) return GESPMM_EINVAL;
    int kind = 0;
    const int rc = gespmm::run_spmm_x16(nullptr, nullptr, nullptr, nullptr, nullptr, GESPMM_X16_BF16, M, K, N, nnz, variant, 0, nullptr, nullptr,
                                        b_align, c_align, true, &kind);
    if (rc != 0 && rc != gespmm::kX16Unavailable) return rc < 0 ? rc : GESPMM_EINVAL;
    return kind;
}

// The multi-head product (gespmm.h): the heads kernel where it exists, else the composition — per head, gather the head's weights and
// its slice of B into stream-ordered temporaries, the strict-order product into a third, scatter that into C. Same bits: each head IS
// that product. H = 1 is the strict-order product on the caller's arrays.
int gespmm_csr_spmm_heads_f32(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B, float* C, int64_t M,
                              int64_t K, int64_t H, int64_t F, int64_t nnz, void* stream) {
    const int rc0 = gespmm::check_heads_args(rowptr, colind, val, B, C, M, K, H, F, nnz);
    if (rc0 != 0) return rc0;
    if (M == 0 || F == 0) return 0;
    int kind = 0;
    int rc = gespmm::run_spmm_heads(rowptr, colind, val, B, C, M, K, H, F, nnz, GESPMM_VARIANT_AUTO, 0, stream, nullptr,
                                    gespmm::pointer_alignment(B), gespmm::pointer_alignment(C), false, &kind);
    if (rc != gespmm::kHeadsUnavailable) return rc;
    const gespmm_launch_cfg strict = {0, 0, 0, 0, 0, GESPMM_FLAG_STRICT_ORDER};
    if (H == 1) return run_spmm(rowptr, colind, val, B, C, M, K, F, nnz, GESPMM_VARIANT_AUTO, &strict, gespmm::kReduceSum, 0.0f, stream);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if ((rc = gespmm::refuse_allocation_under_capture(st)) != 0) return rc;  // (nothing launched)
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t v_bytes = up((size_t)nnz * 4), b_bytes = up((size_t)K * (size_t)F * 4), c_bytes = (size_t)M * (size_t)F * 4;
    void* scratch = nullptr;
    hipError_t e = gespmm::workspace_alloc(&scratch, v_bytes + b_bytes + c_bytes, st);
    if (e != hipSuccess) return (int)e;
    float* vh = static_cast<float*>(scratch);
    float* Bh = reinterpret_cast<float*>(static_cast<char*>(scratch) + v_bytes);
    float* Ch = reinterpret_cast<float*>(static_cast<char*>(scratch) + v_bytes + b_bytes);
    const int64_t N = H * F;
    rc = 0;
    for (int64_t h = 0; h < H && rc == 0; ++h) {  // (stream order keeps one head's temporaries until its scatter has read them)
        rc = (int)gespmm::launch_heads_slice(val, vh, nnz, H, h, 1, st);
        if (rc == 0 && nnz != 0) rc = (int)gespmm::launch_heads_slice(B, Bh, K, N, h * F, F, st);
        if (rc == 0) rc = run_spmm(rowptr, colind, vh, Bh, Ch, M, K, F, nnz, GESPMM_VARIANT_AUTO, &strict, gespmm::kReduceSum, 0.0f, stream);
        if (rc == 0) rc = (int)gespmm::launch_heads_unslice(Ch, C, M, N, h * F, F, st);
    }
    e = gespmm::workspace_free(scratch, st);
    if (rc == 0) rc = (int)e;
    return rc;
}

int gespmm_heads_route(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, int b_align, int c_align, int32_t* geometry_out) {
    if (b_align < 1 || c_align < 1) return GESPMM_EINVAL;
    const int rc0 = gespmm::check_heads_sizes(M, K, H, F, nnz);
    if (rc0 != 0) return rc0;
    int kind = 0;
    gespmm::Geometry geo = {};
    const int rc = gespmm::run_spmm_heads(nullptr, nullptr, nullptr, nullptr, nullptr, M, K, H, F, nnz, GESPMM_VARIANT_AUTO, 0, nullptr, nullptr,
                                          b_align, c_align, true, &kind, &geo);
    if (rc != 0 && rc != gespmm::kHeadsUnavailable) return rc < 0 ? rc : GESPMM_EINVAL;
    if (geometry_out) {
        geometry_out[0] = kind ? geo.vec : 0;
        geometry_out[1] = kind ? geo.strips : 0;
        geometry_out[2] = kind ? geo.group : 0;
        geometry_out[3] = kind ? geo.rows_per_wave : 0;
    }
    return kind;
}

int gespmm_csr_spmm_f32_cfg(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B,
                            float* C, int64_t M, int64_t K, int64_t N, int64_t nnz, int variant,
                            const gespmm_launch_cfg* cfg, void* stream) {
    return run_spmm(rowptr, colind, val, B, C, M, K, N, nnz, variant, cfg, gespmm::kReduceSum, 0.0f, stream);
}

int gespmm_csr_spmm_max_f32(const int32_t* rowptr, const int32_t* colind, const float* B, float* C, int64_t M,
                            int64_t K, int64_t N, int64_t nnz, float empty_value, int variant, void* stream) {
    if (gespmm::auto_plan_enabled() && variant != GESPMM_VARIANT_NAIVE && variant != GESPMM_VARIANT_PARREDUCE) {
        int rc = 0;
        if (check_common(rowptr, colind, nullptr, B, C, M, K, N, nnz) == 0 && variant >= GESPMM_VARIANT_AUTO && variant < GESPMM_NUM_VARIANTS &&
            gespmm::auto_plan_try(rowptr, colind, nullptr, B, C, M, K, N, nnz, variant, gespmm::kReduceMax, empty_value, stream, &rc))
            return rc;
    }
    return run_spmm(rowptr, colind, nullptr, B, C, M, K, N, nnz, variant, nullptr, gespmm::kReduceMax, empty_value,
                    stream);
}

int64_t gespmm_csr_spmm_workspace_bytes(int64_t M, int64_t K, int64_t N, int64_t nnz, int variant,
                                        const gespmm_launch_cfg* cfg) {
    if (M < 0 || K < 0 || N < 0 || nnz < -1) return GESPMM_EINVAL;
    if (variant < GESPMM_VARIANT_AUTO || variant >= GESPMM_NUM_VARIANTS) return GESPMM_EINVAL;
    if (M == 0 || N == 0) return 0;
    // the geometry depends on the alignment of B and C, unknown here: take the largest need
    size_t need = 0;
    for (int max_vec = 1; max_vec <= 4; max_vec *= 2) {
        if (N % max_vec != 0) break;
        gespmm::Selection sel;
        if (gespmm::resolve_geometry(M, K, N, nnz, variant, max_vec, cfg ? cfg->vec : 0, cfg ? cfg->strips : 0,
                                     cfg ? cfg->group : 0, cfg ? cfg->rows_per_wave : 0, cfg ? cfg->slab_rows : 0,
                                     cfg ? cfg->flags : 0, &sel) != 0)
            return GESPMM_EINVAL;
        size_t b = 0;
        if (sel.variant == GESPMM_VARIANT_PARREDUCE || sel.variant == GESPMM_VARIANT_NAIVE) b = 0;
        else if (sel.geo.slab_blocked) b = gespmm::slabblocked_workspace_bytes(M, sel.geo);
        else if (sel.geo.split_long_rows) b = gespmm::longrows_workspace_bytes(nnz, N, sel.geo.long_row_threshold);
        if (b > need) need = b;
    }
    return (int64_t)need;
}

int gespmm_csr_spmm_f32_ws(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B, float* C,
                           int64_t M, int64_t K, int64_t N, int64_t nnz, int variant, const gespmm_launch_cfg* cfg,
                           void* workspace, int64_t workspace_bytes, void* stream) {
    if (workspace_bytes < 0 || (workspace_bytes > 0 && workspace == nullptr)) return GESPMM_EINVAL;
    // no launch knobs (no cfg, or every field 0 — what the torch op passes): the stateless call with the caller's scratch
    const bool no_knobs = cfg == nullptr || (cfg->vec == 0 && cfg->strips == 0 && cfg->group == 0 && cfg->rows_per_wave == 0 &&
                                             cfg->slab_rows == 0 && cfg->flags == 0);
    if (no_knobs && gespmm::auto_plan_enabled()) {
        int rc = 0;
        if (check_common(rowptr, colind, val, B, C, M, K, N, nnz) == 0 && variant >= GESPMM_VARIANT_AUTO && variant < GESPMM_NUM_VARIANTS &&
            variant != GESPMM_VARIANT_NAIVE && variant != GESPMM_VARIANT_PARREDUCE &&
            gespmm::auto_plan_try(rowptr, colind, val, B, C, M, K, N, nnz, variant, gespmm::kReduceSum, 0.0f, stream, &rc))
            return rc;
    }
    return run_spmm(rowptr, colind, val, B, C, M, K, N, nnz, variant, cfg, gespmm::kReduceSum, 0.0f, stream, workspace,
                    workspace_bytes);
}

int gespmm_select_variant(int64_t M, int64_t nnz, int64_t N) { return gespmm::auto_variant(M, nnz, N); }

int gespmm_describe_launch(int64_t M, int64_t K, int64_t N, int64_t nnz, int variant, const gespmm_launch_cfg* cfg,
                           char* out, int64_t capacity) {
    if (!out || capacity <= 0 || M < 0 || K < 0 || N < 0 || nnz < -1) return GESPMM_EINVAL;
    if (variant < GESPMM_VARIANT_AUTO || variant >= GESPMM_NUM_VARIANTS) return GESPMM_EINVAL;
    int max_vec = 4;
    while (max_vec > 1 && (N % max_vec) != 0) max_vec >>= 1;
    gespmm::Selection sel;
    const int flags = cfg ? cfg->flags : 0;
    const int rc = gespmm::resolve_geometry(M, K, N, nnz, variant, max_vec, cfg ? cfg->vec : 0, cfg ? cfg->strips : 0,
                                            cfg ? cfg->group : 0, cfg ? cfg->rows_per_wave : 0, cfg ? cfg->slab_rows : 0,
                                            flags, &sel);
    if (rc != 0) return rc;
    const gespmm::Geometry& g = sel.geo;
    const char* idx = g.idx64 ? "idx64" : "idx32";
    int n;
    if (sel.variant == GESPMM_VARIANT_PARREDUCE)
        n = snprintf(out, (size_t)capacity, "variant=5 kernel=parallel-reduction W=%d %s", g.group, idx);
    else if (sel.variant == GESPMM_VARIANT_NAIVE)
        n = snprintf(out, (size_t)capacity, "variant=0 kernel=naive V=%d S=%d W=%d %s", g.vec, g.strips, g.group, idx);
    else if (g.slab_blocked)
        n = snprintf(out, (size_t)capacity, "variant=%d kernel=slab-blocked V=%d S=%d W=%d slab_rows=%d slabs=%lld %s",
                     sel.variant, g.vec, g.strips, g.group, g.slab_rows,
                     (long long)((K + g.slab_rows - 1) / g.slab_rows), idx);
    else {
        bool seg = g.segmented;
        if (flags & gespmm::kFlagBatchStream) seg = false;
        if ((flags & gespmm::kFlagSegStream) && !g.split_long_rows) seg = true;
        char tail[64] = "";
        if (!seg && g.split_long_rows) snprintf(tail, sizeof tail, " long_rows>%d chunk=%d", g.long_row_threshold, gespmm::kLongRowChunk);
        const char* st = (g.sc1_store || (flags & gespmm::kFlagSc1Store)) ? " c_stores=sc1" : "";
        if (seg)
            n = snprintf(out, (size_t)capacity, "variant=%d kernel=segmented-stream V=%d S=%d W=%d rows_per_group=%d %s%s",
                         sel.variant, g.vec, g.strips, g.group, g.rows_per_group, idx, st);
        else
            n = snprintf(out, (size_t)capacity, "variant=%d kernel=batch-stream V=%d S=%d W=%d rows_per_wave=%d %s%s%s",
                         sel.variant, g.vec, g.strips, g.group, g.rows_per_wave, idx, tail, st);
    }
    if (n < 0) return GESPMM_EINVAL;
    return n < capacity ? n : (int)capacity - 1;
}

// DGL hands over neither nnz nor the number of source nodes. For large graphs the 4-byte read of
// indptr[m] (a stream synchronisation — the patch's CustomCsrmm synchronises the stream right after the
// kernel anyway, binary_reduce_sum.cu:358) buys the dense-graph and long-row paths: reddit-shaped,
// N=128: 8.3 -> 4.2 ms. The number of source nodes is taken as m for the slab count only (columns beyond
// it fall into the last slab — same result), offsets into B stay 64-bit. Not on a capturing stream.
// Rows from which the DGL entry points read nnz back (a stream synchronisation); < 0 = never. Process-wide, set
// once at start-up by the integrator (gespmm_dgl_set_readback_rows).
static std::atomic<int64_t> g_dgl_readback_rows{1 << 15};

int gespmm_dgl_set_readback_rows(int64_t rows) {
    g_dgl_readback_rows.store(rows, std::memory_order_relaxed);
    return 0;
}

static int dgl_csrmm(int m, int n, const int32_t* indptr, const int32_t* indices, const float* B, float* C, int reduce,
                     float empty, void* stream) {
    int64_t nnz = -1, K = 0x7fffffffLL;
    gespmm_launch_cfg cfg = {0, 0, 0, 0, 0, 0};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (gespmm::auto_plan_enabled() && m > 0 && n > 0 && indptr && indices && B && C) {
        // (the fingerprint's read-back is the synchronisation this entry point performs anyway; K and nnz come out of it)
        int rc = 0;
        if (gespmm::auto_plan_try(indptr, indices, nullptr, B, C, m, 0, n, -1, GESPMM_VARIANT_AUTO, reduce, empty, stream, &rc)) return rc;
    }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
    const int64_t rb_rows = g_dgl_readback_rows.load(std::memory_order_relaxed);
    if (!capturing && rb_rows >= 0 && m >= rb_rows && indptr) {
        int32_t last = -1;
        if (hipMemcpyAsync(&last, indptr + m, sizeof last, hipMemcpyDeviceToHost, st) == hipSuccess &&
            hipStreamSynchronize(st) == hipSuccess && last >= 0) {
            nnz = last;
            K = m;
            cfg.flags = GESPMM_FLAG_FORCE_IDX64;
        }
    }
    (void)hipGetLastError();
    return run_spmm(indptr, indices, nullptr, B, C, m, K, n, nnz, GESPMM_VARIANT_AUTO, &cfg, reduce, empty, stream);
}

int gespmm_dgl_csrmm_sum_f32(int m, int n, const int32_t* indptr, const int32_t* indices, const float* B, float* C,
                             void* stream) {
    return dgl_csrmm(m, n, indptr, indices, B, C, gespmm::kReduceSum, 0.0f, stream);
}

int gespmm_dgl_csrmm_max_f32(int m, int n, const int32_t* indptr, const int32_t* indices, const float* B, float* C,
                             void* stream) {
    return dgl_csrmm(m, n, indptr, indices, B, C, gespmm::kReduceMax, -10000.0f, stream);
}

int gespmm_sddmm_coo_f32(const int32_t* rowind, const int32_t* colind, const float* D1, const float* D2, float* out,
                         int64_t nnz, int64_t N, void* stream) {
    if (nnz < 0 || N < 0) return GESPMM_EINVAL;
    if (nnz > gespmm::kSddmmMaxNnz || N > 0x7fffffffLL / 4) return GESPMM_ERANGE;
    if (nnz == 0) return 0;
    if (!rowind || !colind || !out || (N > 0 && (!D1 || !D2))) return GESPMM_EINVAL;
    if (!aligned_to(rowind, 4) || !aligned_to(colind, 4) || !aligned_to(D1, 4) || !aligned_to(D2, 4) ||
        !aligned_to(out, 4))
        return GESPMM_EALIGN;
    return (int)gespmm::launch_sddmm(rowind, false, colind, D1, D2, out, 0, nnz, N,
                                     reinterpret_cast<hipStream_t>(stream));
}

int gespmm_sddmm_csr_f32(const int32_t* rowptr, const int32_t* colind, const float* D1, const float* D2, float* out,
                         int64_t M, int64_t nnz, int64_t N, void* stream) {
    if (M < 0 || nnz < 0 || N < 0) return GESPMM_EINVAL;
    if (M > 0x7fffffffLL - 1 || nnz > gespmm::kSddmmMaxNnz || N > 0x7fffffffLL / 4) return GESPMM_ERANGE;
    if (nnz == 0) return 0;
    if (!rowptr || !colind || !out || (N > 0 && (!D1 || !D2))) return GESPMM_EINVAL;
    if (!aligned_to(rowptr, 4) || !aligned_to(colind, 4) || !aligned_to(D1, 4) || !aligned_to(D2, 4) ||
        !aligned_to(out, 4))
        return GESPMM_EALIGN;
    return (int)gespmm::launch_sddmm(rowptr, true, colind, D1, D2, out, M, nnz, N,
                                     reinterpret_cast<hipStream_t>(stream));
}

// 16-bit operands (fp16 / bf16 D1 and D2, fp32 out): the checks of the two entry points above, in their order, with the dtype
// among the arguments that must make sense and D1 / D2 on 2-byte boundaries.
static bool sddmm_x16_dtype(int dtype) { return dtype == GESPMM_X16_F16 || dtype == GESPMM_X16_BF16; }

int gespmm_sddmm_coo_x16(const int32_t* rowind, const int32_t* colind, const void* D1, const void* D2, float* out, int dtype,
                         int64_t nnz, int64_t N, void* stream) {
    if (nnz < 0 || N < 0 || !sddmm_x16_dtype(dtype)) return GESPMM_EINVAL;
    if (nnz > gespmm::kSddmmMaxNnz || N > 0x7fffffffLL / 4) return GESPMM_ERANGE;
    if (nnz == 0) return 0;
    if (!rowind || !colind || !out || (N > 0 && (!D1 || !D2))) return GESPMM_EINVAL;
    if (!aligned_to(rowind, 4) || !aligned_to(colind, 4) || !aligned_to(D1, 2) || !aligned_to(D2, 2) || !aligned_to(out, 4))
        return GESPMM_EALIGN;
    return (int)gespmm::launch_sddmm_x16(rowind, false, colind, D1, D2, out, dtype, 0, nnz, N, reinterpret_cast<hipStream_t>(stream));
}

int gespmm_sddmm_csr_x16(const int32_t* rowptr, const int32_t* colind, const void* D1, const void* D2, float* out, int dtype,
                         int64_t M, int64_t nnz, int64_t N, void* stream) {
    if (M < 0 || nnz < 0 || N < 0 || !sddmm_x16_dtype(dtype)) return GESPMM_EINVAL;
    if (M > 0x7fffffffLL - 1 || nnz > gespmm::kSddmmMaxNnz || N > 0x7fffffffLL / 4) return GESPMM_ERANGE;
    if (nnz == 0) return 0;
    if (!rowptr || !colind || !out || (N > 0 && (!D1 || !D2))) return GESPMM_EINVAL;
    if (!aligned_to(rowptr, 4) || !aligned_to(colind, 4) || !aligned_to(D1, 2) || !aligned_to(D2, 2) || !aligned_to(out, 4))
        return GESPMM_EALIGN;
    return (int)gespmm::launch_sddmm_x16(rowptr, true, colind, D1, D2, out, dtype, M, nnz, N, reinterpret_cast<hipStream_t>(stream));
}

static int describe_sddmm(int csr, int64_t M, int64_t nnz, int64_t N, int d1_align, int d2_align, int capturing, char* out,
                          int64_t capacity, int elem_size) {
    if (!out || capacity <= 0 || M < 0 || nnz < 0 || N < 0) return GESPMM_EINVAL;
    if (d1_align < elem_size || d2_align < elem_size || (d1_align & (d1_align - 1)) != 0 || (d2_align & (d2_align - 1)) != 0)
        return GESPMM_EINVAL;
    if (M > 0x7fffffffLL - 1 || nnz > gespmm::kSddmmMaxNnz || N > 0x7fffffffLL / 4) return GESPMM_ERANGE;
    int n;
    if (nnz == 0) {
        n = snprintf(out, (size_t)capacity, "form=none");
    } else {
        const gespmm::SddmmLaunch r = gespmm::resolve_sddmm(csr != 0, M, nnz, N, d1_align > 16 ? 16 : d1_align,
                                                           d2_align > 16 ? 16 : d2_align, capturing != 0, elem_size);
        if (r.form == gespmm::kSddmmBlocked)
            n = snprintf(out, (size_t)capacity, "form=blocked V=%d W=%d nslab=%lld slab_rows=%lld", r.V, r.W, (long long)r.nslab,
                         (long long)r.slab_rows);
        else if (r.form == gespmm::kSddmmRowWalk)
            n = snprintf(out, (size_t)capacity, "form=row-walk V=%d W=%d", r.V, r.W);
        else
            n = snprintf(out, (size_t)capacity, "form=%s V=%d W=%d epw=%d", r.form == gespmm::kSddmmCsrEdge ? "csr-edge" : "coo-edge",
                         r.V, r.W, r.epw);
    }
    if (n < 0) return GESPMM_EINVAL;
    return n < capacity ? n : (int)capacity - 1;
}

int gespmm_describe_sddmm(int csr, int64_t M, int64_t nnz, int64_t N, int d1_align, int d2_align, int capturing, char* out,
                          int64_t capacity) {
    return describe_sddmm(csr, M, nnz, N, d1_align, d2_align, capturing, out, capacity, 4);
}

int gespmm_describe_sddmm_x16(int csr, int64_t M, int64_t nnz, int64_t N, int d1_align, int d2_align, int capturing, char* out,
                              int64_t capacity) {
    return describe_sddmm(csr, M, nnz, N, d1_align, d2_align, capturing, out, capacity, 2);
}

// The multi-head SDDMM (gespmm.h): D1 [., H F], D2 [., H F], out [nnz, H]. The checks of the fp32 entries above, in their order.
int gespmm_sddmm_coo_heads_f32(const int32_t* rowind, const int32_t* colind, const float* D1, const float* D2, float* out, int64_t H,
                               int64_t F, int64_t nnz, void* stream) {
    const int rc = gespmm::check_sddmm_heads_args(rowind, false, colind, D1, D2, out, 0, H, F, nnz);
    if (rc != 0) return rc < 0 ? rc : 0;
    return gespmm::run_sddmm_heads(rowind, false, colind, D1, D2, out, 0, -1, H, F, nnz, stream);
}

int gespmm_sddmm_csr_heads_f32(const int32_t* rowptr, const int32_t* colind, const float* D1, const float* D2, float* out, int64_t M,
                               int64_t H, int64_t F, int64_t nnz, void* stream) {
    const int rc = gespmm::check_sddmm_heads_args(rowptr, true, colind, D1, D2, out, M, H, F, nnz);
    if (rc != 0) return rc < 0 ? rc : 0;
    return gespmm::run_sddmm_heads(rowptr, true, colind, D1, D2, out, M, -1, H, F, nnz, stream);
}

int gespmm_describe_sddmm_heads(int csr, int64_t M, int64_t nnz, int64_t H, int64_t F, int d1_align, int d2_align, int capturing, char* out,
                                int64_t capacity) {
    if (!out || capacity <= 0) return GESPMM_EINVAL;
    if (d1_align < 4 || d2_align < 4 || (d1_align & (d1_align - 1)) != 0 || (d2_align & (d2_align - 1)) != 0) return GESPMM_EINVAL;
    const int rc = gespmm::check_sddmm_heads_sizes(csr != 0, M, H, F, nnz);
    if (rc != 0) return rc;
    int n;
    if (nnz == 0) {
        n = snprintf(out, (size_t)capacity, "form=none");
    } else if (F == 0) {
        n = snprintf(out, (size_t)capacity, "route=zeros");
    } else {
        const gespmm::SddmmHeadsLaunch r = gespmm::resolve_sddmm_heads(csr != 0, M, nnz, H, F, d1_align > 16 ? 16 : d1_align,
                                                                       d2_align > 16 ? 16 : d2_align, capturing != 0, gespmm::sddmm_heads_pin());
        if (r.route == gespmm::kSddmmHeadsPlain) {
            n = snprintf(out, (size_t)capacity, "route=plain ");
            if (n > 0 && n < capacity) {
                const int m = describe_sddmm(csr, M, nnz, F, d1_align, d2_align, capturing, out + n, capacity - n, 4);
                if (m < 0) return m;
                n += m;
            }
        } else if (r.route == gespmm::kSddmmHeadsKernel) {
            n = snprintf(out, (size_t)capacity, "route=kernel form=%s V=%d W=%d epw=%d", r.form == gespmm::kSddmmCsrEdge ? "csr-edge" : "coo-edge",
                         r.V, r.W, r.epw);
        } else {
            n = snprintf(out, (size_t)capacity, "route=composition V=%d W=%d", r.V, r.W);
        }
    }
    if (n < 0) return GESPMM_EINVAL;
    return n < capacity ? n : (int)capacity - 1;
}

/* The edge softmax over CSR rows (gespmm.h). One kernel for every size the checks let through; resolve_edge_softmax decides its shape. */
int gespmm_edge_softmax_f32(const int32_t* rowptr, const float* score, float* out, int64_t M, int64_t H, int64_t nnz, float slope,
                            void* stream) {
    const int rc = gespmm::check_edge_softmax_sizes(M, H, nnz, slope);
    if (rc != 0) return rc;
    if (nnz == 0) return 0;
    if (!rowptr || !score || !out) return GESPMM_EINVAL;
    if (!aligned_to(rowptr, 4) || !aligned_to(score, 4) || !aligned_to(out, 4)) return GESPMM_EALIGN;
    return (int)gespmm::launch_edge_softmax(rowptr, score, out, M, H, nnz, slope, gespmm::resolve_edge_softmax(M, nnz, H),
                                            reinterpret_cast<hipStream_t>(stream));
}

int gespmm_edge_softmax_backward_f32(const int32_t* rowptr, const float* alpha, const float* grad_alpha, const float* score,
                                     float* grad_score, int64_t M, int64_t H, int64_t nnz, float slope, void* stream) {
    const int rc = gespmm::check_edge_softmax_sizes(M, H, nnz, slope);
    if (rc != 0) return rc;
    if (nnz == 0) return 0;
    const bool leaky = slope != 1.0f;  // (score is looked at only then)
    if (!rowptr || !alpha || !grad_alpha || !grad_score || (leaky && !score)) return GESPMM_EINVAL;
    if (!aligned_to(rowptr, 4) || !aligned_to(alpha, 4) || !aligned_to(grad_alpha, 4) || !aligned_to(grad_score, 4) ||
        (leaky && !aligned_to(score, 4)))
        return GESPMM_EALIGN;
    return (int)gespmm::launch_edge_softmax_backward(rowptr, alpha, grad_alpha, leaky ? score : nullptr, grad_score, M, H, nnz, slope,
                                                     gespmm::resolve_edge_softmax(M, nnz, H), reinterpret_cast<hipStream_t>(stream));
}

int gespmm_describe_edge_softmax(int64_t M, int64_t nnz, int64_t H, char* out, int64_t capacity) {
    if (!out || capacity <= 0) return GESPMM_EINVAL;
    const int rc = gespmm::check_edge_softmax_sizes(M, H, nnz, 1.0f);
    if (rc != 0) return rc;
    int n;
    if (nnz == 0) {
        n = snprintf(out, (size_t)capacity, "form=none");
    } else {
        const gespmm::EdgeSoftmaxLaunch r = gespmm::resolve_edge_softmax(M, nnz, H);
        n = snprintf(out, (size_t)capacity, "W=%d long_rows>%d", r.W, r.L);
    }
    if (n < 0) return GESPMM_EINVAL;
    return n < capacity ? n : (int)capacity - 1;
}

int gespmm_baseline_atomic_scatter_f32(const int32_t* rowptr, const int32_t* colind, const float* in, float* out,
                                       int64_t M, int64_t K, int64_t N, int64_t nnz, void* stream) {
    if (M < 0 || K < 0 || N < 0 || nnz < 0) return GESPMM_EINVAL;
    if (M > 0x7fffffffLL - 1 || K > 0x7fffffffLL || N > 0x7fffffffLL / 4 || nnz > 0x7fffffffLL) return GESPMM_ERANGE;
    if (K == 0 || N == 0) return 0;
    if (!out || (nnz > 0 && (!rowptr || !colind || !in))) return GESPMM_EINVAL;
    return (int)gespmm::launch_atomic_scatter(rowptr, colind, in, out, M, K, N, nnz,
                                              reinterpret_cast<hipStream_t>(stream));
}

int gespmm_baseline_copy_f32(const float* src, float* dst, int64_t n, void* stream) {
    if (n < 0) return GESPMM_EINVAL;
    if (n == 0) return 0;
    if (!src || !dst) return GESPMM_EINVAL;
    if (!aligned_to(src, 4) || !aligned_to(dst, 4)) return GESPMM_EALIGN;
    return (int)gespmm::launch_copy(src, dst, n, reinterpret_cast<hipStream_t>(stream));
}

int64_t gespmm_csr2csc_workspace_bytes(int64_t M, int64_t K, int64_t nnz) {
    if (M < 0 || K < 0 || nnz < 0) return GESPMM_EINVAL;
    return gespmm::csr2csc_workspace_bytes(M, K, nnz);
}

int gespmm_csr2csc_f32(const int32_t* rowptr, const int32_t* colind, const float* csr_val, int32_t* colptr,
                       int32_t* rowind, float* csc_val, int64_t M, int64_t K, int64_t nnz, void* workspace,
                       void* stream) {
    if (M < 0 || K < 0 || nnz < 0) return GESPMM_EINVAL;
    if (M > 0x7fffffffLL - 1 || K > 0x7fffffffLL - 1 || nnz > 0x7fffffffLL) return GESPMM_ERANGE;
    if (!rowptr || !colptr) return GESPMM_EINVAL;
    if (nnz > 0 && (!colind || !rowind || !workspace)) return GESPMM_EINVAL;
    if ((csr_val == nullptr) != (csc_val == nullptr)) return GESPMM_EINVAL;
    return (int)gespmm::launch_csr2csc(rowptr, colind, csr_val, colptr, rowind, csc_val, M, K, nnz, workspace,
                                       reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
