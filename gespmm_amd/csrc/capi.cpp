// capi.cpp — the extern "C" boundary declared in include/gespmm.h.
//
// Argument validation, variant -> launch-geometry selection, and the hand-off to
// the HIP launchers. Nothing here touches device memory; the only HIP calls are
// the kernel launches themselves. There is deliberately no CPU fallback: on a
// machine without a HIP device the launch fails and its hipError_t is returned.
//
// How the file is laid out: the shared pieces first — argument checks, the capture query, resolve_stream_launch (the ONE place that
// decides which streaming kernel runs, in which lane geometry, with which flags) and PooledScratch (the ONE temporary of a stateless
// composition) — then one short function per product that shows what is particular to it, then the entry points.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/gespmm.h"
#include "select.h"
#include "auto_plan.h"
#include "edge_dropout.h"
#include "edge_softmax.h"
#include "gat_aggregate.h"
#include "gat_backward.h"
#include "dot_attention.h"
#include "dot_attention_x16.h"
#include "gatv2_attention.h"
#include "gatv2_attention_x16.h"
#include "gatv2_score.h"
#include "plan.h"
#include "sddmm_heads.h"
#include "spmm_heads.h"
#include "spmm_max_arg.h"
#include "spmm_kernels.h"
#include "workspace.h"

namespace gespmm {

int check_csr_sizes(int64_t M, int64_t K, int64_t N, int64_t nnz, int64_t min_nnz) {
    if (M < 0 || K < 0 || N < 0 || nnz < min_nnz) return GESPMM_EINVAL;
    if (M > kMaxRows || K > kMaxCols || N > kMaxWidth || nnz > kMaxNnz) return GESPMM_ERANGE;
    return 0;
}

int check_sddmm_sizes(bool csr, int64_t M, int64_t nnz, int64_t N) {
    if (nnz < 0 || N < 0 || (csr && M < 0)) return GESPMM_EINVAL;
    if ((csr && M > kSddmmMaxRows) || nnz > kSddmmMaxNnz || N > kMaxWidth) return GESPMM_ERANGE;
    return 0;
}

int check_pointers(std::initializer_list<PointerArg> args) {
    for (const PointerArg& a : args)
        if (a.required && !a.p) return GESPMM_EINVAL;
    for (const PointerArg& a : args)
        if (reinterpret_cast<uintptr_t>(a.p) % (uintptr_t)a.elem != 0) return GESPMM_EALIGN;
    return 0;
}

// ---- the multi-head product (gespmm.h: gespmm_csr_spmm_heads_f32): H F, the width, within what the other entries take as N
int check_heads_sizes(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz) {
    if (H < 1) return GESPMM_EINVAL;
    const int rc = check_csr_sizes(M, K, F, nnz, 0);
    if (rc != 0) return rc;
    return (H > kMaxWidth || F > kMaxWidth / H) ? GESPMM_ERANGE : 0;
}

// ... and the multi-head SDDMM: the COO form has no composition to take a pair count past the kernel's limit
int check_sddmm_heads_sizes(bool csr, int64_t M, int64_t H, int64_t F, int64_t nnz) {
    if (H < 1) return GESPMM_EINVAL;
    const int rc = check_sddmm_sizes(csr, M, nnz, F);
    if (rc != 0) return rc;
    return (H > kMaxWidth || F > kMaxWidth / H || (!csr && nnz > kSddmmMaxNnz / H)) ? GESPMM_ERANGE : 0;
}

int pointer_alignment(const void* p) {
    int a = 16;
    while (a > 1 && reinterpret_cast<uintptr_t>(p) % (uintptr_t)a != 0) a >>= 1;
    return a;
}

int vec_limit(int64_t unit, int align) {
    int max_vec = 4;
    while (max_vec > 1 && ((unit % max_vec) != 0 || align < 4 * max_vec)) max_vec >>= 1;
    return max_vec;
}

Capture stream_capture(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) return Capture::QueryFailed;
    return cs != hipStreamCaptureStatusNone ? Capture::Yes : Capture::No;
}

bool is_capturing(hipStream_t st) {
    if (stream_capture(st) == Capture::Yes) return true;
    (void)hipGetLastError();
    return false;
}

int refuse_allocation_under_capture(hipStream_t st) { return is_capturing(st) ? (int)hipErrorStreamCaptureUnsupported : 0; }

int resolve_stream_launch(const StreamQuery& q, StreamLaunch* out) {
    int flags = q.flags;
    // Under stream capture the paths that need a stream-ordered temporary are switched off: a
    // captured allocation becomes a mem-alloc graph node, and replaying those costs seconds per
    // launch on this runtime (measured: 14 s per GCN epoch on reddit-like instead of 20 ms).
    // The streaming kernels need no workspace and give the same bits (slab path) or the strict
    // CSR-order chain (long-row pass).
    if (q.ask_stream && is_capturing(q.stream)) {
        flags |= kFlagNoSlabBlocked | kFlagStrictOrder;
        flags &= ~(kFlagSlabBlocked | kFlagSplitLongRows);
    }
    const PlanLaunch* pl = q.tables;
    if (pl) {  // task tables exist for the two streaming kernels only
        flags |= kFlagNoSlabBlocked;
        flags &= ~(kFlagSlabBlocked | kFlagSegStream | kFlagBatchStream);
        flags |= (pl->prefer_segmented && pl->gtasks) ? kFlagSegStream : kFlagBatchStream;
        flags &= ~kFlagAllowReassoc;  // a plan runs the CRC family only (the parallel-reduction variant has no task table)
    }
    const gespmm_launch_cfg none = {0, 0, 0, 0, 0, 0};
    const gespmm_launch_cfg& k = q.knobs ? *q.knobs : none;
    const int rc = resolve_geometry(q.M, q.K, q.N, q.nnz, q.variant, q.max_vec, k.vec, k.strips, k.group, k.rows_per_wave, k.slab_rows, flags,
                                    &out->sel);
    if (rc != 0) return rc;
    Geometry& g = out->sel.geo;
    g.reduce = q.reduce;
    bool seg = g.segmented;
    if (flags & kFlagBatchStream) seg = false;
    if ((flags & kFlagSegStream) && !g.split_long_rows) seg = true;
    // operands that are only 4- or 8-byte aligned resolve to a narrower vector; two strips of < 4 floats have no
    // segmented-stream instantiation: a plan then runs its wavefront task table (any N and alignment stay legal)
    if (seg && pl && g.strips == 2 && g.vec < 4) seg = false;
    out->flags = flags;
    out->segmented = seg;
    out->rpw = seg ? g.rows_per_group : g.rows_per_wave;
    return (out->sel.variant == GESPMM_VARIANT_NAIVE || out->sel.variant == GESPMM_VARIANT_PARREDUCE) ? kNotStreaming : 0;
}

}  // namespace gespmm

namespace {

using namespace gespmm;

// The arguments of a streaming launch that every product fills the same way: the matrix, the operands, the resolved flags and rows per
// wavefront, the plan's task tables. Everything else is zero.
template <class ARGS>
ARGS stream_args(const CsrView& A, const float* B, float* C, int64_t N, const StreamLaunch& r) {
    ARGS a = {};
    a.rowptr = A.rowptr;
    a.colind = A.colind;
    a.val = A.val;
    a.B = B;
    a.C = C;
    a.M = (int32_t)A.M;
    a.N = (int32_t)N;
    a.flags = r.flags;
    a.rpw = r.rpw;
    if (const PlanLaunch* pl = A.tables()) {
        a.tasks = pl->tasks;
        a.perm = pl->perm;
        a.ntasks = pl->ntasks;
        a.gtasks = pl->gtasks;
        a.ngtasks = pl->ngtasks;
    }
    return a;
}

// The stream-ordered temporary of a stateless composition: ONE block from the library's pool, handed out in slices that start on
// 256-byte boundaries, freed once.
struct PooledScratch {
    hipStream_t st = nullptr;
    char* base = nullptr;
    size_t used = 0;
    static size_t slice(size_t bytes) { return (bytes + 255) & ~(size_t)255; }  // what a slice takes of the block when another follows it
    // hipErrorStreamCaptureUnsupported on a capturing stream (nothing is allocated, the caller launches nothing), or the pool's error
    int open(size_t bytes, hipStream_t stream) {
        st = stream;
        const int rc = refuse_allocation_under_capture(st);
        return rc != 0 ? rc : (int)workspace_alloc(reinterpret_cast<void**>(&base), bytes, st);
    }
    // like: the slice starts address(like) % 16 bytes past its boundary — the caller's alignment class, hence the caller's V
    float* take(size_t bytes, const void* like = nullptr) {
        float* p = reinterpret_cast<float*>(base + used + reinterpret_cast<uintptr_t>(like) % 16);
        used += slice(bytes);
        return p;
    }
    int close(int rc) {  // the first error wins
        if (!base) return rc;
        const hipError_t e = workspace_free(base, st);
        return rc != 0 ? rc : (int)e;
    }
};

int check_common(const int32_t* rowptr, const int32_t* colind, const float* val, const void* B, const void* C, int64_t M, int64_t K, int64_t N,
                 int64_t nnz, int dense_elem = 4) {
    const int rc = check_csr_sizes(M, K, N, nnz, -1);
    if (rc != 0) return rc;
    if (M == 0 || N == 0) return 0;  // nothing to do; pointers may be null
    return check_pointers({{rowptr, 4, true}, {C, dense_elem, true}, {colind, 4, nnz != 0}, {B, dense_elem, nnz != 0}, {val, 4, false}});
}

}  // namespace

namespace gespmm {

int run_spmm(const CsrView& A, const float* B, float* C, int64_t N, const gespmm_launch_cfg* cfg, int reduce, float empty, void* stream,
             void* ws, int64_t ws_bytes, const LaunchGuard* guard) {
    const int64_t M = A.M, nnz = A.nnz;
    const int rc = check_common(A.rowptr, A.colind, A.val, B, C, M, A.K, N, nnz);
    if (rc != 0) return rc;
    if (M == 0 || N == 0) return 0;
    if (!valid_variant(A.variant)) return GESPMM_EINVAL;
    if (reduce == kReduceMax && (A.val != nullptr || A.variant == GESPMM_VARIANT_PARREDUCE || A.variant == GESPMM_VARIANT_NAIVE))
        return GESPMM_EINVAL;
    if (cfg && (cfg->rows_per_wave < 0 || cfg->rows_per_wave > kMaxRowsPerWave || cfg->slab_rows < 0)) return GESPMM_EINVAL;

    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // with the caller's workspace nothing is allocated whether capturing or not: the stream is not asked (a workspace that turns out
    // too small falls back to the pool — gespmm_csr_spmm_workspace_bytes is an upper bound)
    const bool callers_scratch = ws != nullptr && ws_bytes > 0;
    const size_t ws_size = (size_t)(ws_bytes > 0 ? ws_bytes : 0);
    const PlanLaunch* pl = A.tables();
    // Vector width is limited by what both B and C rows can be addressed with.
    const StreamQuery q = {M, A.K, N, nnz, vec_limit(N, min_alignment(B, C)), A.variant, cfg ? cfg->flags : 0, reduce, pl, cfg, !callers_scratch, st};
    StreamLaunch r;
    const int src = resolve_stream_launch(q, &r);
    if (src == kNotStreaming && pl) return GESPMM_EINVAL;  // (task tables exist for the two streaming kernels only)
    if (src != 0 && src != kNotStreaming) return src;
    const Selection& sel = r.sel;

    SpmmArgs a = stream_args<SpmmArgs>(A, B, C, N, r);
    a.flags |= sel.geo.sc1_store ? kFlagSc1Store : 0;
    a.empty = empty;
    a.guard = guard ? guard->word : nullptr;
    a.guard_want = guard ? guard->want : 0;
    // a guard covers ONE kernel: the two streaming kernels without the long-row pass
    if (guard && (src == kNotStreaming || sel.geo.slab_blocked || sel.geo.split_long_rows)) return kNotGuardable;
    if (guard && guard->word == nullptr) return 0;  // dry run (auto_plan.cpp): would this call be one guardable kernel? nothing is launched

    if (sel.variant == GESPMM_VARIANT_PARREDUCE) return (int)launch_spmm_parreduce(a, sel.geo, st);
    if (sel.variant == GESPMM_VARIANT_NAIVE) return (int)launch_spmm_naive(a, sel.geo, st);
    if (sel.geo.slab_blocked) {
        // rows per lane group and launch: 2 measured best on reddit-like at N = 64..256 (hub rows make
        // 8-row tasks a long tail: 45 % average occupancy in the PMC run), profiles/r01/slab_task_size.log
        a.rpw = (cfg && cfg->rows_per_wave > 0) ? cfg->rows_per_wave : 2;
        return (int)launch_spmm_slabblocked(a, sel.geo, ws, ws_size, st);
    }
    if (r.segmented) return (int)launch_spmm_segstream(a, sel.geo, st);
    if (!sel.geo.split_long_rows) return (int)launch_spmm_stream(a, sel.geo, st);
    a.long_row = sel.geo.long_row_threshold;
    return (int)launch_spmm_stream_with_longrows(a, sel.geo, nnz, ws, ws_size, st);
}

// The fused counterpart of run_spmm: the same selection (a plan's task tables included), then ONE fused streaming kernel or nothing.
// The stream is never asked; V is also limited by the bias slice (the bits do not depend on it).
int run_spmm_fused(const CsrView& A, const float* B, const FusedVectors& fx, float* C, int64_t N, int flags, void* stream, bool dry_run,
                   int* kind) {
    *kind = 0;
    if (!valid_variant(A.variant)) return GESPMM_EINVAL;
    if (A.M <= 0 || N <= 0) return kFusedUnavailable;
    const int align = dry_run ? 16 : std::min(min_alignment(B, C), pointer_alignment(fx.bias));
    const StreamQuery q = {A.M, A.K, N, A.nnz, vec_limit(N, align), A.variant, flags, kReduceSum, A.tables(), nullptr, false, nullptr};
    StreamLaunch r;
    const int rc = resolve_stream_launch(q, &r);
    if (rc != 0) return rc == kNotStreaming ? kFusedUnavailable : GESPMM_EINVAL;
    if (!fused_geometry_served(r.sel.geo, r.segmented, A.planned)) return kFusedUnavailable;  // (long-row pass, cache blocking, 64-bit offsets too)
    *kind = r.segmented ? 2 : 1;
    if (dry_run) return 0;
    FusedSpmmArgs a = stream_args<FusedSpmmArgs>(A, B, C, N, r);
    a.col_scale = fx.col_scale;
    a.row_scale = fx.row_scale;
    a.bias = fx.bias;
    return (int)launch_spmm_fused(a, r.sel.geo, r.segmented, reinterpret_cast<hipStream_t>(stream));
}

// The 16-bit counterpart: ONE 16-bit streaming kernel or nothing (kX16Unavailable: the caller composes widen, the fp32 route, narrow).
// The kernels work in 32-bit words, so the geometry is the one the selector resolves for the byte-equivalent fp32 width N / 2 — every
// rule of select.cpp is about bytes and lanes per row — with V limited by what B and C can be addressed with, in words. Unless dry, a
// capturing stream takes the streaming kernels, which allocate nothing (as run_spmm without a workspace).
int run_spmm_x16(const CsrView& A, const void* B, void* C, int dtype, int64_t N, int flags, void* stream, int b_align, int c_align,
                 bool dry_run, int* kind, Geometry* geo_out) {
    *kind = 0;
    if (!valid_variant(A.variant)) return GESPMM_EINVAL;
    if (A.M <= 0 || N <= 0 || N % 2 != 0 || b_align < 4 || c_align < 4) return kX16Unavailable;
    const int64_t Nw = N / 2;  // words per row
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const StreamQuery q = {A.M, A.K, Nw, A.nnz, vec_limit(Nw, std::min(b_align, c_align)), A.variant, flags, kReduceSum, A.tables(), nullptr, !dry_run, st};
    StreamLaunch r;
    const int rc = resolve_stream_launch(q, &r);
    if (rc != 0) return rc == kNotStreaming ? kX16Unavailable : GESPMM_EINVAL;
    if (!x16_geometry_served(r.sel.geo, r.segmented, A.planned)) return kX16Unavailable;  // (long-row pass, cache blocking, 64-bit offsets too)
    *kind = r.segmented ? 2 : 1;
    if (geo_out) *geo_out = r.sel.geo;
    if (dry_run) return 0;
    // (arrays of words: spmm_kernels.h, HalfSpmmArgs)
    const SpmmArgs a = stream_args<SpmmArgs>(A, static_cast<const float*>(B), static_cast<float*>(C), Nw, r);
    return (int)launch_spmm_x16(a, dtype, r.sel.geo, r.segmented, st);
}

// The multi-head counterpart: ONE heads kernel or nothing (kHeadsUnavailable: the caller composes per head). The geometry is what the
// selector resolves for width N = H F with the batch-stream kernel forced, strict order and no cache blocking; V is limited to what
// divides F (a lane's vector stays inside one head) and to what B and C can be addressed with. The stream is never asked.
int run_spmm_heads(const CsrView& A, const float* B, float* C, int64_t H, int64_t F, int flags, void* stream, int b_align, int c_align,
                   bool dry_run, int* kind, Geometry* geo_out, const int32_t* order) {
    *kind = 0;
    if (!valid_variant(A.variant)) return GESPMM_EINVAL;
    if (H < 2 || H > kHeadsMax || A.M <= 0 || F <= 0 || A.nnz < 0 || b_align < 4 || c_align < 4) return kHeadsUnavailable;
    // GESPMM_HEADS_ROUTE=composition pins route 0 (read per call: scripts/heads_timing.py measures both routes in one process)
    if (const char* env = getenv("GESPMM_HEADS_ROUTE"))
        if (!strcmp(env, "composition")) return kHeadsUnavailable;
    const int64_t N = H * F;
    if ((uint64_t)A.K * (uint64_t)N * 4ull >= (1ull << 32) || A.nnz * H >= (1ll << 31)) return kHeadsUnavailable;  // 32-bit offsets only
    flags |= kFlagBatchStream | kFlagStrictOrder | kFlagNoSlabBlocked;
    flags &= ~(kFlagSegStream | kFlagSlabBlocked | kFlagSplitLongRows | kFlagAllowReassoc | kFlagForceIdx64);
    const StreamQuery q = {A.M, A.K, N, A.nnz, vec_limit(F, std::min(b_align, c_align)), A.variant, flags, kReduceSum, A.tables(), nullptr, false, nullptr};
    StreamLaunch r;
    const int rc = resolve_stream_launch(q, &r);
    if (rc != 0) return rc == kNotStreaming ? kHeadsUnavailable : GESPMM_EINVAL;
    if (!heads_geometry_served(r.sel.geo, A.planned)) return kHeadsUnavailable;
    *kind = 1;
    if (geo_out) *geo_out = r.sel.geo;
    if (dry_run) return 0;
    if (A.nnz != 0 && (!A.val || !A.colind || !B)) return GESPMM_EINVAL;  // (no entries: the kernel reads none of the three and writes zeros)
    HeadsArgs a = stream_args<HeadsArgs>(A, B, C, N, r);
    a.H = (int32_t)H;
    a.F = (int32_t)F;
    // (through an edge order: the ordered kernels, storage order only — a plan composes the order into its own copy of the weights)
    if (order) return A.planned ? GESPMM_EINVAL : (int)launch_spmm_heads_order(a, order, 0, r.sel.geo, reinterpret_cast<hipStream_t>(stream));
    return (int)launch_spmm_heads(a, r.sel.geo, reinterpret_cast<hipStream_t>(stream));
}

// ... and on 16-bit B and C (gespmm_csr_spmm_heads_x16): ONE 16-bit heads kernel or nothing (kHeadsUnavailable: the caller composes widen,
// the fp32 entry, narrow). The kernel works in 32-bit words, so the geometry is run_spmm_heads's for H heads of F / 2 WORDS: the width
// H F / 2, V limited to what divides F / 2 and to what B and C can be addressed with. Storage order only; the stream is never asked.
int run_spmm_heads_x16(const CsrView& A, const void* B, void* C, int dtype, int64_t H, int64_t F, void* stream, int b_align, int c_align,
                       bool dry_run, int* kind, Geometry* geo_out, const int32_t* order = nullptr) {
    *kind = 0;
    if (H < 2 || H > kHeadsMax || A.M <= 0 || F <= 0 || F % 2 != 0 || A.nnz < 0 || b_align < 4 || c_align < 4) return kHeadsUnavailable;
    // GESPMM_HEADS_X16_ROUTE=composition pins route 0 (read per call: scripts/heads_x16_timing.py measures both routes in one process)
    if (const char* env = getenv("GESPMM_HEADS_X16_ROUTE"))
        if (!strcmp(env, "composition")) return kHeadsUnavailable;
    const int64_t Fw = F / 2, Nw = H * Fw;  // words per head, words per row
    if ((uint64_t)A.K * (uint64_t)Nw * 4ull >= (1ull << 32) || A.nnz * H >= (1ll << 31)) return kHeadsUnavailable;  // 32-bit offsets only
    const int flags = kFlagBatchStream | kFlagStrictOrder | kFlagNoSlabBlocked;
    const StreamQuery q = {A.M, A.K, Nw, A.nnz, vec_limit(Fw, std::min(b_align, c_align)), GESPMM_VARIANT_AUTO, flags, kReduceSum, nullptr, nullptr, false, nullptr};
    StreamLaunch r;
    const int rc = resolve_stream_launch(q, &r);
    if (rc != 0) return rc == kNotStreaming ? kHeadsUnavailable : GESPMM_EINVAL;
    if (!heads_geometry_served(r.sel.geo, false)) return kHeadsUnavailable;
    *kind = 1;
    if (geo_out) *geo_out = r.sel.geo;
    if (dry_run) return 0;
    if (A.nnz != 0 && (!A.val || !A.colind || !B)) return GESPMM_EINVAL;  // (no entries: the kernel reads none of the three and writes zeros)
    // (arrays of words: spmm_heads.h)
    HeadsArgs a = stream_args<HeadsArgs>(A, static_cast<const float*>(B), static_cast<float*>(C), Nw, r);
    a.H = (int32_t)H;
    a.F = (int32_t)Fw;
    if (order) return (int)launch_spmm_heads_order(a, order, dtype, r.sel.geo, reinterpret_cast<hipStream_t>(stream));
    return (int)launch_spmm_heads_x16(a, dtype, r.sel.geo, reinterpret_cast<hipStream_t>(stream));
}

// The fused GAT aggregation (gat_aggregate.h): ONE kernel or nothing (kHeadsUnavailable: the caller materialises the weights and calls
// the multi-head product). A is the pattern the segments come from — (rowptr, colind) with M rows, or (colptr, rowind) with K — and
// A.K the rows of B; the geometry is run_spmm_heads's, H = 1 included. The stream is never asked.
int check_gat_softmax_sizes(int64_t M, int64_t K, int64_t H, int64_t nnz, float slope);  // (below, with the softmax's other checks)
int run_gat_aggregate(const CsrView& A, const GatTerms& t, const float* B, float* C, int64_t H, int64_t F, bool transposed, void* stream,
                      int b_align, int c_align, bool dry_run, int* kind, Geometry* geo_out, const EdgeDropout* drop = nullptr) {
    *kind = 0;
    if (H < 1 || H > kHeadsMax || A.M <= 0 || F <= 0 || A.nnz < 0 || b_align < 4 || c_align < 4) return kHeadsUnavailable;
    // GESPMM_GAT_AGGREGATE_ROUTE=composition pins route 0 (read per call: scripts/gat_aggregate_timing.py measures both in one process)
    if (const char* env = getenv("GESPMM_GAT_AGGREGATE_ROUTE"))
        if (!strcmp(env, "composition")) return kHeadsUnavailable;
    const int64_t N = H * F;
    if ((uint64_t)A.K * (uint64_t)N * 4ull >= (1ull << 32) || A.nnz * H >= (1ll << 31)) return kHeadsUnavailable;  // 32-bit offsets only
    const int flags = kFlagBatchStream | kFlagStrictOrder | kFlagNoSlabBlocked;
    const StreamQuery q = {A.M, A.K, N, A.nnz, vec_limit(F, std::min(b_align, c_align)), A.variant, flags, kReduceSum, nullptr, nullptr, false, nullptr};
    StreamLaunch r;
    const int rc = resolve_stream_launch(q, &r);
    if (rc != 0) return rc == kNotStreaming ? kHeadsUnavailable : GESPMM_EINVAL;
    if (!heads_geometry_served(r.sel.geo, false)) return kHeadsUnavailable;
    *kind = 1;
    if (geo_out) *geo_out = r.sel.geo;
    if (dry_run) return 0;
    GatAggregateArgs a = stream_args<GatAggregateArgs>(A, B, C, N, r);
    a.H = (int32_t)H;
    a.F = (int32_t)F;
    a.el = t.el;
    a.er = t.er;
    a.stats = t.stats;
    a.slope = t.slope;
    return (int)launch_gat_aggregate(a, r.sel.geo, transposed, drop, reinterpret_cast<hipStream_t>(stream));
}

// gespmm_gat_aggregate_f32 / gespmm_gat_aggregate_route: the ladder of gespmm_gat_softmax_f32 on (M, K, H, nnz), then the multi-head
// product's on the width (segments x rows of B: M x K, transposed K x M)
int check_gat_aggregate_sizes(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, bool transposed) {
    if (F < 0) return GESPMM_EINVAL;
    const int rc = check_gat_softmax_sizes(M, K, H, nnz, slope);
    if (rc != 0) return rc;
    return check_heads_sizes(transposed ? K : M, transposed ? M : K, H, F, nnz);
}

// ---- dropout on the attention coefficients (gespmm.h: gespmm_edge_dropout_f32 and the *_dropout_f32 forms; edge_dropout.h). A bad p joins
// the step of the base entry's ladder that rejects a bad slope: `rc` is what the base's size checks said.
int check_dropout_p(int rc, float p) {
    if (rc == GESPMM_EINVAL || !(p >= 0.0f && p < 1.0f)) return GESPMM_EINVAL;
    return rc;
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

// ... and the dense [rows, H] operands and results of the fused forms (el, er, grad_el, the segment sums): 32-bit word positions too
int check_dense_words(int64_t rows, int64_t H) { return rows > kSddmmMaxNnz / H ? GESPMM_ERANGE : 0; }

// gespmm_gat_softmax_f32 / _backward_f32: the softmax's own checks and K — what makes no sense before what is too large
int check_gat_softmax_sizes(int64_t M, int64_t K, int64_t H, int64_t nnz, float slope) {
    const int rc = check_edge_softmax_sizes(M, H, nnz, slope);
    if (rc == GESPMM_EINVAL || K < 1) return GESPMM_EINVAL;
    if (rc != 0) return rc;
    if (const int rcm = check_dense_words(M, H)) return rcm;
    return check_dense_words(K, H);
}

// gespmm_gat_backward_el_f32 / _er_f32: the ladder of gespmm_gat_aggregate_f32 in both directions, then the 32-bit word positions of the
// two [*, H, F] operands (no other route takes what the kernel cannot address)
int check_gat_backward_sizes(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope) {
    int rc = check_gat_aggregate_sizes(M, K, H, F, nnz, slope, false);
    if (rc == 0) rc = check_gat_aggregate_sizes(M, K, H, F, nnz, slope, true);
    if (rc != 0 || F == 0) return rc;
    if (const int rcm = check_dense_words(M, H * F)) return rcm;  // (H F <= kMaxWidth: no overflow)
    return check_dense_words(K, H * F);
}

// One multi-head SDDMM on checked arguments, nnz > 0: what resolve_sddmm_heads answers, nothing else.
//   plain        H == 1: launch_sddmm on the caller's arrays.
//   kernel       one sddmm_heads_kernel; never allocates.
//   composition  CSR only (past the kernel's pair limit, or pinned). Per head: D1[:, hF:(h+1)F] and D2[:, hF:(h+1)F] into stream-ordered temporaries that start address(D) % 16
//                bytes past a 256-byte boundary — the caller's alignment class, hence the caller's V — launch_sddmm at width F into an
//                nnz temporary, scatter into out[:, h]. K < 0: the call does not say how many rows D2 has; 1 + the largest column index
//                is found on the device and read back (one stream synchronisation; a plan passes its K).
// dtype 0: fp32 operands; kX16F16 / kX16Bf16: 16-bit operands (gespmm_sddmm_*_heads_x16) — the same routes at element size 2, every launch
// the 16-bit one, the slices 2-byte copies.
static int run_sddmm_heads_elem(const int32_t* rows, bool csr, const int32_t* colind, const void* D1v, const void* D2v, float* out, int dtype,
                                int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, void* stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool x16 = dtype != 0;
    const size_t es = x16 ? 2 : 4;
    const float* D1 = static_cast<const float*>(D1v);  // (looked at through these names on the fp32 path only)
    const float* D2 = static_cast<const float*>(D2v);
    // one single-head launch on contiguous operands, of either element type
    auto single = [&](const void* d1, const void* d2, float* o) {
        return x16 ? (int)launch_sddmm_x16(rows, csr, colind, d1, d2, o, dtype, M, nnz, F, st)
                   : (int)launch_sddmm(rows, csr, colind, static_cast<const float*>(d1), static_cast<const float*>(d2), o, M, nnz, F, st);
    };
    if (F == 0) return (int)hipMemsetAsync(out, 0, (size_t)nnz * (size_t)H * sizeof(float), st);
    const bool capturing = stream_capture(st) != Capture::No;  // (a failed query counts as capturing)
    (void)hipGetLastError();
    const SddmmHeadsLaunch r = resolve_sddmm_heads(csr, M, nnz, H, F, pointer_alignment(D1v), pointer_alignment(D2v), capturing, sddmm_heads_pin(),
                                                   (int)es);
    if (r.route == kSddmmHeadsPlain) return single(D1v, D2v, out);
    if (r.route == kSddmmHeadsKernel)
        return x16 ? (int)launch_sddmm_heads_x16(rows, colind, D1v, D2v, out, dtype, M, nnz, H, F, r, st)
                   : (int)launch_sddmm_heads(rows, colind, D1, D2, out, M, nnz, H, F, r, st);
    if (!csr) return GESPMM_ERANGE;  // (check_sddmm_heads_sizes lets no such call through)
    int rc = 0;
    if (K < 0) {
        PooledScratch probe;
        int32_t h_max = 0;
        if ((rc = probe.open(256, st)) != 0) return rc;  // (nothing launched)
        int32_t* d_max = reinterpret_cast<int32_t*>(probe.take(256));
        hipError_t e = launch_max_index(colind, nnz, d_max, st);
        if (e == hipSuccess) e = hipMemcpyAsync(&h_max, d_max, sizeof h_max, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if ((rc = probe.close((int)e)) != 0) return rc;
        K = (int64_t)h_max + 1;
    }
    const size_t d1_bytes = (size_t)M * (size_t)F * es + 16, d2_bytes = (size_t)K * (size_t)F * es + 16, t_bytes = (size_t)nnz * 4;
    PooledScratch scratch;
    if ((rc = scratch.open(PooledScratch::slice(d1_bytes) + PooledScratch::slice(d2_bytes) + t_bytes, st)) != 0) return rc;  // (nothing launched)
    float* D1h = scratch.take(d1_bytes, D1v);
    float* D2h = scratch.take(d2_bytes, D2v);
    float* th = scratch.take(t_bytes);
    const int64_t N = H * F;
    for (int64_t h = 0; h < H && rc == 0; ++h) {  // (stream order keeps one head's temporaries until its scatter has read them)
        rc = x16 ? (int)launch_heads_slice_x16(D1v, D1h, M, N, h * F, F, st) : (int)launch_heads_slice(D1, D1h, M, N, h * F, F, st);
        if (rc == 0) rc = x16 ? (int)launch_heads_slice_x16(D2v, D2h, K, N, h * F, F, st) : (int)launch_heads_slice(D2, D2h, K, N, h * F, F, st);
        if (rc == 0) rc = single(D1h, D2h, th);
        if (rc == 0) rc = (int)launch_heads_unslice(th, out, nnz, H, h, 1, st);
    }
    return scratch.close(rc);
}

int run_sddmm_heads(const int32_t* rows, bool csr, const int32_t* colind, const float* D1, const float* D2, float* out, int64_t M, int64_t K,
                    int64_t H, int64_t F, int64_t nnz, void* stream) {
    return run_sddmm_heads_elem(rows, csr, colind, D1, D2, out, 0, M, K, H, F, nnz, stream);
}

// ---- the GATv2 score (gespmm.h: gespmm_gatv2_score_f32 / _backward_f32; gatv2_score.h). S segments of x_seg, T rows of x_ind (forward:
// M and K). Sizes alone: what makes no sense, then what is too large for 32-bit word positions (there is no other route).
int check_gatv2_sizes(int64_t S, int64_t T, int64_t H, int64_t F, int64_t nnz, float slope) {
    const int rc = check_edge_softmax_sizes(S, H, nnz, slope);
    if (rc == GESPMM_EINVAL || T < 0 || F < 0 || (nnz > 0 && T < 1)) return GESPMM_EINVAL;
    if (rc != 0) return rc;
    if (S > kSddmmMaxNnz || T > kSddmmMaxNnz) return GESPMM_ERANGE;
    if (const int rcs = check_dense_words(S, H)) return rcs;
    if (const int rct = check_dense_words(T, H)) return rct;
    if (F == 0) return 0;
    if (const int rcs = check_dense_words(S * H, F)) return rcs;  // (S H <= kSddmmMaxNnz: no overflow)
    return check_dense_words(T * H, F);
}

// ---- the fused dot-product attention (gespmm.h: gespmm_dot_attention_f32 and its backward; dot_attention.h). Sizes alone: what makes no
// sense (a scale that is no finite number and a bad p with it), what is too large for 32-bit word positions — the GATv2 ladder, and the
// [M, H, 2] words of stats — then the slice no kernel serves.
int check_dot_attention_sizes(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, const float* p) {
    int rc = check_gatv2_sizes(M, K, H, F, nnz, scale);
    if (p) rc = check_dropout_p(rc, *p);
    if (rc != 0) return rc;
    if (const int rcs = check_dense_words(M * H, 2)) return rcs;  // (M H <= kSddmmMaxNnz: no overflow)
    return F > kDotAttentionMaxF ? GESPMM_ERR_UNSUPPORTED : 0;
}

// ---- the fused GATv2 attention (gespmm.h: gespmm_gatv2_attention_f32 and its backward; gatv2_attention.h): the same ladder with the
// slope in the scale's place.
int check_gatv2_attention_sizes(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, const float* p) {
    int rc = check_gatv2_sizes(M, K, H, F, nnz, slope);
    if (p) rc = check_dropout_p(rc, *p);
    if (rc != 0) return rc;
    if (const int rcs = check_dense_words(M * H, 2)) return rcs;  // (M H <= kSddmmMaxNnz: no overflow)
    return F > kGatv2AttentionMaxF ? GESPMM_ERR_UNSUPPORTED : 0;
}

int least_alignment(std::initializer_list<const void*> ps) {
    int align = 16;
    for (const void* p : ps) align = std::min(align, pointer_alignment(p));
    return align;
}

}  // namespace gespmm

namespace {
int run_spmm(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B, float* C, int64_t M,
             int64_t K, int64_t N, int64_t nnz, int variant, const gespmm_launch_cfg* cfg, int reduce, float empty,
             void* stream, void* ws = nullptr, int64_t ws_bytes = 0) {
    return gespmm::run_spmm(csr_view(rowptr, colind, val, M, K, nnz, variant), B, C, N, cfg, reduce, empty, stream, ws, ws_bytes);
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
        case GESPMM_ERR_UNSUPPORTED: return "gespmm: no kernel serves this shape (fused dot-product attention: F <= 512)";
    }
    if (code > 0) return hipGetErrorString((hipError_t)code);
    return "gespmm: unknown error code";
}

int gespmm_csr_spmm_f32(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B, float* C,
                        int64_t M, int64_t K, int64_t N, int64_t nnz, int variant, void* stream) {
    if (gespmm::auto_plan_enabled()) {  // (gespmm_set_auto_plan: off by default — one relaxed load)
        int rc = 0;
        if (check_common(rowptr, colind, val, B, C, M, K, N, nnz) == 0 && valid_variant(variant) &&
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
    const FusedVectors fx = {col_scale, row_scale, bias};
    int rc = check_common(rowptr, colind, val, B, C, M, K, N, nnz);
    if (rc == 0) rc = check_pointers({{col_scale, 4, false}, {row_scale, 4, false}, {bias, 4, false}});
    if (rc != 0) return rc;
    if (!valid_variant(variant)) return GESPMM_EINVAL;
    if (M == 0 || N == 0) return 0;
    if (!fx.any()) return gespmm_csr_spmm_f32(rowptr, colind, val, B, C, M, K, N, nnz, variant, stream);
    int kind = 0;
    rc = run_spmm_fused(csr_view(rowptr, colind, val, M, K, nnz, variant), B, fx, C, N, 0, stream, false, &kind);
    if (rc != kFusedUnavailable) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    PooledScratch scratch;
    const float* Bin = B;
    if (col_scale && K > 0 && nnz != 0) {
        const size_t b_bytes = (size_t)K * (size_t)N * 4;
        if ((rc = scratch.open(b_bytes, st)) != 0) return rc;  // (nothing launched)
        float* Bs = scratch.take(b_bytes);
        if ((rc = (int)launch_scale_rows(B, col_scale, Bs, K, N, st)) != 0) return scratch.close(rc);
        Bin = Bs;
    }
    rc = run_spmm(rowptr, colind, val, Bin, C, M, K, N, nnz, variant, nullptr, kReduceSum, 0.0f, stream);
    if (rc == 0) rc = (int)launch_scale_bias_inplace(C, row_scale, bias, M, N, st);
    return scratch.close(rc);
}

// 16-bit dense operands (gespmm.h): one 16-bit streaming kernel where the byte-equivalent fp32 call would be one streaming kernel, else
// the composition — widen B into a stream-ordered temporary, the fp32 call unchanged into a second one, narrow into C. Same bits:
// widening is exact and either way the fp32 sum is rounded once.
int gespmm_csr_spmm_x16(const int32_t* rowptr, const int32_t* colind, const float* val, const void* B, void* C, int dtype, int64_t M,
                        int64_t K, int64_t N, int64_t nnz, int variant, void* stream) {
    if (!valid_x16_dtype(dtype)) return GESPMM_EINVAL;
    int rc = check_common(rowptr, colind, val, B, C, M, K, N, nnz, 2);
    if (rc != 0) return rc;
    if (!valid_variant(variant)) return GESPMM_EINVAL;
    if (M == 0 || N == 0) return 0;
    int kind = 0;
    rc = run_spmm_x16(csr_view(rowptr, colind, val, M, K, nnz, variant), B, C, dtype, N, 0, stream, pointer_alignment(B), pointer_alignment(C),
                      false, &kind);
    if (rc != kX16Unavailable) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t b_bytes = (size_t)K * (size_t)N * 4, c_bytes = (size_t)M * (size_t)N * 4;
    PooledScratch scratch;
    if ((rc = scratch.open(PooledScratch::slice(b_bytes) + c_bytes, st)) != 0) return rc;  // (nothing launched)
    float* Bf = scratch.take(b_bytes);
    float* Cf = scratch.take(c_bytes);
    if (B && nnz != 0) rc = (int)launch_widen_x16(B, Bf, dtype, K * N, st);
    if (rc == 0) rc = run_spmm(rowptr, colind, val, Bf, Cf, M, K, N, nnz, variant, nullptr, kReduceSum, 0.0f, stream);
    if (rc == 0) rc = (int)launch_narrow_x16(Cf, C, dtype, M * N, st);
    return scratch.close(rc);
}

int gespmm_x16_route(int64_t M, int64_t K, int64_t N, int64_t nnz, int variant, int b_align, int c_align) {
    if (M < 0 || K < 0 || N < 0 || nnz < -1 || b_align < 1 || c_align < 1) return GESPMM_EINVAL;
    if (!valid_variant(variant)) return GESPMM_EINVAL;
    int kind = 0;
    const int rc = run_spmm_x16(csr_view(nullptr, nullptr, nullptr, M, K, nnz, variant), nullptr, nullptr, GESPMM_X16_BF16, N, 0, nullptr, b_align,
                                c_align, true, &kind);
    return route_result(rc == kX16Unavailable ? 0 : rc, kind);
}

// The multi-head product (gespmm.h): the heads kernel where it exists, else the composition — per head, gather the head's weights and
// its slice of B into stream-ordered temporaries, the strict-order product into a third, scatter that into C. Same bits: each head IS
// that product. H = 1 is the strict-order product on the caller's arrays.
int gespmm_csr_spmm_heads_f32(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B, float* C, int64_t M,
                              int64_t K, int64_t H, int64_t F, int64_t nnz, void* stream) {
    int rc = check_heads_sizes(M, K, H, F, nnz);
    if (rc != 0) return rc;
    if (M == 0 || F == 0) return 0;
    rc = check_pointers({{rowptr, 4, true}, {C, 4, true}, {colind, 4, nnz != 0}, {B, 4, nnz != 0}, {val, 4, nnz != 0}});
    if (rc != 0) return rc;
    int kind = 0;
    rc = run_spmm_heads(csr_view(rowptr, colind, val, M, K, nnz, GESPMM_VARIANT_AUTO), B, C, H, F, 0, stream, pointer_alignment(B),
                        pointer_alignment(C), false, &kind);
    if (rc != kHeadsUnavailable) return rc;
    const gespmm_launch_cfg strict = {0, 0, 0, 0, 0, GESPMM_FLAG_STRICT_ORDER};
    if (H == 1) return run_spmm(rowptr, colind, val, B, C, M, K, F, nnz, GESPMM_VARIANT_AUTO, &strict, kReduceSum, 0.0f, stream);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t v_bytes = (size_t)nnz * 4, b_bytes = (size_t)K * (size_t)F * 4, c_bytes = (size_t)M * (size_t)F * 4;
    PooledScratch scratch;
    if ((rc = scratch.open(PooledScratch::slice(v_bytes) + PooledScratch::slice(b_bytes) + c_bytes, st)) != 0) return rc;  // (nothing launched)
    float* vh = scratch.take(v_bytes);
    float* Bh = scratch.take(b_bytes);
    float* Ch = scratch.take(c_bytes);
    const int64_t N = H * F;
    for (int64_t h = 0; h < H && rc == 0; ++h) {  // (stream order keeps one head's temporaries until its scatter has read them)
        rc = (int)launch_heads_slice(val, vh, nnz, H, h, 1, st);
        if (rc == 0 && nnz != 0) rc = (int)launch_heads_slice(B, Bh, K, N, h * F, F, st);
        if (rc == 0) rc = run_spmm(rowptr, colind, vh, Bh, Ch, M, K, F, nnz, GESPMM_VARIANT_AUTO, &strict, kReduceSum, 0.0f, stream);
        if (rc == 0) rc = (int)launch_heads_unslice(Ch, C, M, N, h * F, F, st);
    }
    return scratch.close(rc);
}

int gespmm_heads_route(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, int b_align, int c_align, int32_t* geometry_out) {
    if (b_align < 1 || c_align < 1) return GESPMM_EINVAL;
    const int rc0 = check_heads_sizes(M, K, H, F, nnz);
    if (rc0 != 0) return rc0;
    int kind = 0;
    Geometry geo = {};
    const int rc = run_spmm_heads(csr_view(nullptr, nullptr, nullptr, M, K, nnz, GESPMM_VARIANT_AUTO), nullptr, nullptr, H, F, 0, nullptr, b_align,
                                  c_align, true, &kind, &geo);
    const int route = route_result(rc == kHeadsUnavailable ? 0 : rc, kind);
    if (route >= 0 && geometry_out) {
        geometry_out[0] = kind ? geo.vec : 0;
        geometry_out[1] = kind ? geo.strips : 0;
        geometry_out[2] = kind ? geo.group : 0;
        geometry_out[3] = kind ? geo.rows_per_wave : 0;
    }
    return route;
}

// The multi-head product on 16-bit operands (gespmm.h): the 16-bit heads kernel where it exists, else the composition — widen B into a
// stream-ordered temporary, gespmm_csr_spmm_heads_f32 unchanged into a second one, narrow into C. Same bits: widening is exact and either
// way each fp32 chain is rounded once.
int gespmm_csr_spmm_heads_x16(const int32_t* rowptr, const int32_t* colind, const float* val, const void* B, void* C, int dtype, int64_t M,
                              int64_t K, int64_t H, int64_t F, int64_t nnz, void* stream) {
    if (!valid_x16_dtype(dtype)) return GESPMM_EINVAL;
    int rc = check_heads_sizes(M, K, H, F, nnz);
    if (rc != 0) return rc;
    if (M == 0 || F == 0) return 0;
    rc = check_pointers({{rowptr, 4, true}, {C, 2, true}, {colind, 4, nnz != 0}, {B, 2, nnz != 0}, {val, 4, nnz != 0}});
    if (rc != 0) return rc;
    int kind = 0;
    rc = run_spmm_heads_x16(csr_view(rowptr, colind, val, M, K, nnz, GESPMM_VARIANT_AUTO), B, C, dtype, H, F, stream, pointer_alignment(B),
                            pointer_alignment(C), false, &kind, nullptr);
    if (rc != kHeadsUnavailable) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t N = H * F;
    const size_t b_bytes = (size_t)K * (size_t)N * 4, c_bytes = (size_t)M * (size_t)N * 4;
    PooledScratch scratch;
    if ((rc = scratch.open(PooledScratch::slice(b_bytes) + c_bytes, st)) != 0) return rc;  // (nothing launched)
    float* Bf = scratch.take(b_bytes);
    float* Cf = scratch.take(c_bytes);
    if (B && nnz != 0) rc = (int)launch_widen_x16(B, Bf, dtype, K * N, st);
    if (rc == 0) rc = gespmm_csr_spmm_heads_f32(rowptr, colind, val, Bf, Cf, M, K, H, F, nnz, stream);
    if (rc == 0) rc = (int)launch_narrow_x16(Cf, C, dtype, M * N, st);
    return scratch.close(rc);
}

// The multi-head product with its weights read through an edge order (gespmm.h). order == NULL: the unordered entry, nothing else. The
// ordered kernel exists exactly where the unordered one does (run_spmm_heads / run_spmm_heads_x16 answer for the same sizes and
// alignments); everywhere else — and under GESPMM_HEADS_ORDER_ROUTE=composition, read per call (scripts/heads_order_timing.py measures
// both routes in one process) — the composition: gather val through order into a stream-ordered temporary (launch_edge_gather), then the
// unordered entry on it. Same bits: the kernel's row loop is the unordered kernel's on the same staged weights.
static bool heads_order_pinned() {
    const char* env = getenv("GESPMM_HEADS_ORDER_ROUTE");
    return env && !strcmp(env, "composition");
}

// dtype 0: fp32 B and C; kX16F16 / kX16Bf16: 16-bit ones. Checked arguments, order != NULL, nnz > 0.
static int heads_order_entry(const int32_t* rowptr, const int32_t* colind, const int32_t* order, const float* val, const void* B, void* C,
                             int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, void* stream) {
    int rc = kHeadsUnavailable, kind = 0;
    if (!heads_order_pinned()) {
        const CsrView A = csr_view(rowptr, colind, val, M, K, nnz, GESPMM_VARIANT_AUTO);
        rc = dtype == 0 ? run_spmm_heads(A, static_cast<const float*>(B), static_cast<float*>(C), H, F, 0, stream, pointer_alignment(B),
                                         pointer_alignment(C), false, &kind, nullptr, order)
                        : run_spmm_heads_x16(A, B, C, dtype, H, F, stream, pointer_alignment(B), pointer_alignment(C), false, &kind, nullptr, order);
    }
    if (rc != kHeadsUnavailable) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t v_bytes = (size_t)nnz * (size_t)H * 4;
    PooledScratch scratch;
    if ((rc = scratch.open(v_bytes, st)) != 0) return rc;  // (nothing launched; a capturing stream: what every allocating composition returns)
    float* vo = scratch.take(v_bytes);
    rc = (int)launch_edge_gather(val, order, false, vo, nnz, H * 4, st);
    if (rc == 0)
        rc = dtype == 0 ? gespmm_csr_spmm_heads_f32(rowptr, colind, vo, static_cast<const float*>(B), static_cast<float*>(C), M, K, H, F, nnz, stream)
                        : gespmm_csr_spmm_heads_x16(rowptr, colind, vo, B, C, dtype, M, K, H, F, nnz, stream);
    return scratch.close(rc);
}

int gespmm_csr_spmm_heads_order_f32(const int32_t* rowptr, const int32_t* colind, const int32_t* order, const float* val, const float* B,
                                    float* C, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, void* stream) {
    if (!order) return gespmm_csr_spmm_heads_f32(rowptr, colind, val, B, C, M, K, H, F, nnz, stream);
    int rc = check_heads_sizes(M, K, H, F, nnz);
    if (rc != 0) return rc;
    if (M == 0 || F == 0) return 0;
    rc = check_pointers({{rowptr, 4, true}, {C, 4, true}, {colind, 4, nnz != 0}, {B, 4, nnz != 0}, {val, 4, nnz != 0}, {order, 4, false}});
    if (rc != 0) return rc;
    if (nnz == 0) return gespmm_csr_spmm_heads_f32(rowptr, nullptr, nullptr, nullptr, C, M, K, H, F, 0, stream);  // C = 0, no edge array is read
    return heads_order_entry(rowptr, colind, order, val, B, C, 0, M, K, H, F, nnz, stream);
}

int gespmm_csr_spmm_heads_order_x16(const int32_t* rowptr, const int32_t* colind, const int32_t* order, const float* val, const void* B,
                                    void* C, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, void* stream) {
    if (!order) return gespmm_csr_spmm_heads_x16(rowptr, colind, val, B, C, dtype, M, K, H, F, nnz, stream);
    if (!valid_x16_dtype(dtype)) return GESPMM_EINVAL;
    int rc = check_heads_sizes(M, K, H, F, nnz);
    if (rc != 0) return rc;
    if (M == 0 || F == 0) return 0;
    rc = check_pointers({{rowptr, 4, true}, {C, 2, true}, {colind, 4, nnz != 0}, {B, 2, nnz != 0}, {val, 4, nnz != 0}, {order, 4, false}});
    if (rc != 0) return rc;
    if (nnz == 0) return gespmm_csr_spmm_heads_x16(rowptr, nullptr, nullptr, nullptr, C, dtype, M, K, H, F, 0, stream);
    return heads_order_entry(rowptr, colind, order, val, B, C, dtype, M, K, H, F, nnz, stream);
}

// out[i, :] = x[order[i], :] (gespmm.h): the gather behind graphs.take_edges and behind the composition above.
int gespmm_edge_gather(const void* x, const void* order, int order_is_64, void* out, int64_t n, int64_t row_bytes, void* stream) {
    if (n < 0 || row_bytes < 4 || row_bytes % 4 != 0 || row_bytes > 64 || (order_is_64 != 0 && order_is_64 != 1)) return GESPMM_EINVAL;
    if (n > kMaxNnz) return GESPMM_ERANGE;
    if (n == 0) return 0;
    const int rc = check_pointers({{x, 4, true}, {out, 4, true}, {order, order_is_64 ? 8 : 4, true}});
    if (rc != 0) return rc;
    return (int)launch_edge_gather(x, order, order_is_64 != 0, out, n, row_bytes, reinterpret_cast<hipStream_t>(stream));
}

int gespmm_heads_x16_route(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, int b_align, int c_align, int32_t* geometry_out) {
    if (b_align < 1 || c_align < 1) return GESPMM_EINVAL;
    const int rc0 = check_heads_sizes(M, K, H, F, nnz);
    if (rc0 != 0) return rc0;
    int kind = 0;
    Geometry geo = {};
    const int rc = run_spmm_heads_x16(csr_view(nullptr, nullptr, nullptr, M, K, nnz, GESPMM_VARIANT_AUTO), nullptr, nullptr, GESPMM_X16_BF16, H, F,
                                      nullptr, b_align, c_align, true, &kind, &geo);
    const int route = route_result(rc == kHeadsUnavailable ? 0 : rc, kind);
    if (route >= 0 && geometry_out) {
        geometry_out[0] = kind ? geo.vec : 0;
        geometry_out[1] = kind ? geo.strips : 0;
        geometry_out[2] = kind ? geo.group : 0;
        geometry_out[3] = kind ? geo.rows_per_wave : 0;
    }
    return route;
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
        if (check_common(rowptr, colind, nullptr, B, C, M, K, N, nnz) == 0 && valid_variant(variant) &&
            gespmm::auto_plan_try(rowptr, colind, nullptr, B, C, M, K, N, nnz, variant, gespmm::kReduceMax, empty_value, stream, &rc))
            return rc;
    }
    return run_spmm(rowptr, colind, nullptr, B, C, M, K, N, nnz, variant, nullptr, gespmm::kReduceMax, empty_value,
                    stream);
}

/* The max reducer with argmax and its gradient (gespmm.h; spmm_max_arg.h): one kernel each, the batch-stream walk in the geometry the
   selector resolves for (segments, width) with strict order and no cache blocking. S segments (M forward, K backward), T rows of the
   gathered operand (K forward, M backward). There is no second route: what the kernels' 32-bit byte offsets cannot address is refused. */
static int max_arg_sizes(int64_t M, int64_t K, int64_t N, int64_t nnz) {
    const int rc = gespmm::check_csr_sizes(M, K, N, nnz, 0);
    if (rc != 0) return rc;
    if ((uint64_t)K * (uint64_t)N * 4ull >= (1ull << 32) || (uint64_t)M * (uint64_t)N * 4ull >= (1ull << 32)) return GESPMM_ERANGE;
    return 0;
}

static bool ranges_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    if (!a || !b || a_bytes == 0 || b_bytes == 0) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// align: what the three dense operands can be addressed with. dry_run: the geometry alone.
static int max_arg_geometry(int64_t S, int64_t T, int64_t N, int64_t nnz, int align, Geometry* geo) {
    const int flags = kFlagBatchStream | kFlagStrictOrder | kFlagNoSlabBlocked;
    const StreamQuery q = {S, T, N, nnz, vec_limit(N, align), GESPMM_VARIANT_AUTO, flags, kReduceMax, nullptr, nullptr, false, nullptr};
    StreamLaunch r;
    const int rc = resolve_stream_launch(q, &r);
    if (rc != 0) return GESPMM_EINVAL;
    if (!gespmm::max_arg_geometry_served(r.sel.geo)) return GESPMM_ERANGE;
    *geo = r.sel.geo;
    return 0;
}

int gespmm_csr_spmm_max_arg_f32(const int32_t* rowptr, const int32_t* colind, const float* B, float* C, int32_t* arg, int64_t M, int64_t K,
                                int64_t N, int64_t nnz, float empty_value, void* stream) {
    int rc = max_arg_sizes(M, K, N, nnz);
    if (rc == GESPMM_EINVAL || std::isnan(empty_value)) return GESPMM_EINVAL;
    if (rc != 0) return rc;
    if (M == 0 || N == 0) return 0;
    if ((rc = check_pointers({{rowptr, 4, true}, {C, 4, true}, {arg, 4, true}, {colind, 4, nnz != 0}, {B, 4, nnz != 0}})) != 0) return rc;
    const uint64_t b_bytes = (uint64_t)K * (uint64_t)N * 4, c_bytes = (uint64_t)M * (uint64_t)N * 4;
    if (ranges_overlap(C, c_bytes, B, b_bytes) || ranges_overlap(arg, c_bytes, B, b_bytes) || ranges_overlap(C, c_bytes, arg, c_bytes))
        return GESPMM_EINVAL;
    Geometry geo = {};
    const int align = std::min(nnz != 0 ? pointer_alignment(B) : 16, min_alignment(C, arg));
    if ((rc = max_arg_geometry(M, K, N, nnz, align, &geo)) != 0) return rc;
    gespmm::MaxArgArgs a = {};
    a.ptr = rowptr;
    a.ind = colind;
    a.src = B;
    a.dst = C;
    a.arg_out = arg;
    a.S = (int32_t)M;
    a.N = (int32_t)N;
    a.empty = empty_value;
    return (int)gespmm::launch_spmm_max_arg(a, geo, reinterpret_cast<hipStream_t>(stream));
}

int gespmm_csr_spmm_max_backward_f32(const int32_t* colptr, const int32_t* rowind, const int32_t* order, const int32_t* arg,
                                     const float* grad_out, float* grad_B, int64_t M, int64_t K, int64_t N, int64_t nnz, void* stream) {
    int rc = max_arg_sizes(M, K, N, nnz);
    if (rc != 0) return rc;
    if (K == 0 || N == 0) return 0;
    if ((rc = check_pointers({{colptr, 4, true}, {grad_B, 4, true}, {rowind, 4, nnz != 0}, {order, 4, nnz != 0}, {arg, 4, nnz != 0},
                              {grad_out, 4, nnz != 0}})) != 0)
        return rc;
    const uint64_t g_bytes = (uint64_t)K * (uint64_t)N * 4, o_bytes = (uint64_t)M * (uint64_t)N * 4;
    if (ranges_overlap(grad_B, g_bytes, grad_out, o_bytes) || ranges_overlap(grad_B, g_bytes, arg, o_bytes)) return GESPMM_EINVAL;
    Geometry geo = {};
    const int align = std::min(nnz != 0 ? min_alignment(arg, grad_out) : 16, pointer_alignment(grad_B));
    if ((rc = max_arg_geometry(K, M, N, nnz, align, &geo)) != 0) return rc;
    gespmm::MaxArgArgs a = {};
    a.ptr = colptr;
    a.ind = rowind;
    a.order = order;
    a.src = grad_out;
    a.arg_in = arg;
    a.dst = grad_B;
    a.S = (int32_t)K;
    a.N = (int32_t)N;
    return (int)gespmm::launch_spmm_max_backward(a, geo, reinterpret_cast<hipStream_t>(stream));
}

int gespmm_max_arg_route(int64_t M, int64_t nnz, int64_t N, int b_align, int c_align, char* out, int64_t capacity) {
    if (!out || capacity <= 0) return GESPMM_EINVAL;
    for (const int al : {b_align, c_align})
        if (al < 4 || (al & (al - 1)) != 0) return GESPMM_EINVAL;
    const int rc = gespmm::check_csr_sizes(M, 1, N, nnz, 0);
    if (rc != 0) return rc;
    int n;
    if (M == 0 || N == 0) {
        n = snprintf(out, (size_t)capacity, "form=none");
    } else {
        Geometry geo = {};
        // (the lane geometry does not depend on the rows of the gathered operand, once they are within the 32-bit offsets)
        const int rcg = max_arg_geometry(M, 1, N, nnz, std::min(std::min(b_align, c_align), 16), &geo);
        if (rcg != 0) return rcg;
        n = snprintf(out, (size_t)capacity, "V=%d S=%d W=%d", geo.vec, geo.strips, geo.group);
    }
    return describe_result(n, capacity);
}

/* ... on 16-bit dense operands (gespmm.h; spmm_max_arg_x16.hip). The geometry counts ELEMENTS and is the fp32 one at the EFFECTIVE
   alignment: a V-element vector is 2 V bytes of the 16-bit arrays and 4 V bytes of arg, so a 16-bit array aligned to x counts as 2 x.
   The size limits are max_arg_sizes' as they stand: arg is the 4-byte array that sets them. */
static int max_arg_x16_align(int x16_align, int arg_align) { return std::min(std::min(2 * std::min(x16_align, 8), arg_align), 16); }

int gespmm_csr_spmm_max_arg_x16(const int32_t* rowptr, const int32_t* colind, const void* B, void* C, int32_t* arg, int64_t M, int64_t K,
                                int64_t N, int64_t nnz, float empty_value, int dtype, void* stream) {
    if (!valid_x16_dtype(dtype)) return GESPMM_EINVAL;
    int rc = max_arg_sizes(M, K, N, nnz);
    if (rc == GESPMM_EINVAL || std::isnan(empty_value)) return GESPMM_EINVAL;
    if (rc != 0) return rc;
    if (M == 0 || N == 0) return 0;
    if ((rc = check_pointers({{rowptr, 4, true}, {C, 2, true}, {arg, 4, true}, {colind, 4, nnz != 0}, {B, 2, nnz != 0}})) != 0) return rc;
    const uint64_t b_bytes = (uint64_t)K * (uint64_t)N * 2, c_bytes = (uint64_t)M * (uint64_t)N * 2, a_bytes = (uint64_t)M * (uint64_t)N * 4;
    if (ranges_overlap(C, c_bytes, B, b_bytes) || ranges_overlap(arg, a_bytes, B, b_bytes) || ranges_overlap(C, c_bytes, arg, a_bytes))
        return GESPMM_EINVAL;
    Geometry geo = {};
    const int x16_align = std::min(nnz != 0 ? pointer_alignment(B) : 16, pointer_alignment(C));
    if ((rc = max_arg_geometry(M, K, N, nnz, max_arg_x16_align(x16_align, pointer_alignment(arg)), &geo)) != 0) return rc;
    gespmm::MaxArgArgs a = {};
    a.ptr = rowptr;
    a.ind = colind;
    a.src = static_cast<const float*>(B);  // (the 16-bit arrays: spmm_max_arg.h)
    a.dst = static_cast<float*>(C);
    a.arg_out = arg;
    a.S = (int32_t)M;
    a.N = (int32_t)N;
    a.empty = empty_value;
    return (int)gespmm::launch_spmm_max_arg_x16(a, dtype, geo, reinterpret_cast<hipStream_t>(stream));
}

int gespmm_csr_spmm_max_backward_x16(const int32_t* colptr, const int32_t* rowind, const int32_t* order, const int32_t* arg,
                                     const void* grad_out, void* grad_B, int64_t M, int64_t K, int64_t N, int64_t nnz, int dtype,
                                     void* stream) {
    if (!valid_x16_dtype(dtype)) return GESPMM_EINVAL;
    int rc = max_arg_sizes(M, K, N, nnz);
    if (rc != 0) return rc;
    if (K == 0 || N == 0) return 0;
    if ((rc = check_pointers({{colptr, 4, true}, {grad_B, 2, true}, {rowind, 4, nnz != 0}, {order, 4, nnz != 0}, {arg, 4, nnz != 0},
                              {grad_out, 2, nnz != 0}})) != 0)
        return rc;
    const uint64_t g_bytes = (uint64_t)K * (uint64_t)N * 2, o_bytes = (uint64_t)M * (uint64_t)N * 2, a_bytes = (uint64_t)M * (uint64_t)N * 4;
    if (ranges_overlap(grad_B, g_bytes, grad_out, o_bytes) || ranges_overlap(grad_B, g_bytes, arg, a_bytes)) return GESPMM_EINVAL;
    Geometry geo = {};
    const int x16_align = std::min(nnz != 0 ? pointer_alignment(grad_out) : 16, pointer_alignment(grad_B));
    if ((rc = max_arg_geometry(K, M, N, nnz, max_arg_x16_align(x16_align, nnz != 0 ? pointer_alignment(arg) : 16), &geo)) != 0) return rc;
    gespmm::MaxArgArgs a = {};
    a.ptr = colptr;
    a.ind = rowind;
    a.order = order;
    a.src = static_cast<const float*>(grad_out);
    a.arg_in = arg;
    a.dst = static_cast<float*>(grad_B);
    a.S = (int32_t)K;
    a.N = (int32_t)N;
    return (int)gespmm::launch_spmm_max_backward_x16(a, dtype, geo, reinterpret_cast<hipStream_t>(stream));
}

int gespmm_max_arg_route_x16(int64_t M, int64_t nnz, int64_t N, int x16_align, int arg_align, char* out, int64_t capacity) {
    if (!out || capacity <= 0) return GESPMM_EINVAL;
    if (x16_align < 2 || (x16_align & (x16_align - 1)) != 0 || arg_align < 4 || (arg_align & (arg_align - 1)) != 0) return GESPMM_EINVAL;
    const int rc = gespmm::check_csr_sizes(M, 1, N, nnz, 0);
    if (rc != 0) return rc;
    int n;
    if (M == 0 || N == 0) {
        n = snprintf(out, (size_t)capacity, "form=none");
    } else {
        Geometry geo = {};
        const int rcg = max_arg_geometry(M, 1, N, nnz, max_arg_x16_align(x16_align, arg_align), &geo);
        if (rcg != 0) return rcg;
        n = snprintf(out, (size_t)capacity, "V=%d S=%d W=%d", geo.vec, geo.strips, geo.group);
    }
    return describe_result(n, capacity);
}

int64_t gespmm_csr_spmm_workspace_bytes(int64_t M, int64_t K, int64_t N, int64_t nnz, int variant,
                                        const gespmm_launch_cfg* cfg) {
    if (M < 0 || K < 0 || N < 0 || nnz < -1) return GESPMM_EINVAL;
    if (!valid_variant(variant)) return GESPMM_EINVAL;
    if (M == 0 || N == 0) return 0;
    // the geometry depends on the alignment of B and C, unknown here: take the largest need
    size_t need = 0;
    for (int max_vec = 1; max_vec <= 4; max_vec *= 2) {
        if (N % max_vec != 0) break;
        StreamLaunch r;
        const int rc = resolve_stream_launch({M, K, N, nnz, max_vec, variant, cfg ? cfg->flags : 0, kReduceSum, nullptr, cfg, false, nullptr}, &r);
        if (rc != 0 && rc != kNotStreaming) return GESPMM_EINVAL;
        const Geometry& g = r.sel.geo;
        size_t b = 0;
        if (rc == kNotStreaming) b = 0;
        else if (g.slab_blocked) b = slabblocked_workspace_bytes(M, g);
        else if (g.split_long_rows) b = longrows_workspace_bytes(nnz, N, g.long_row_threshold);
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
        if (check_common(rowptr, colind, val, B, C, M, K, N, nnz) == 0 && valid_variant(variant) &&
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
    if (!valid_variant(variant)) return GESPMM_EINVAL;
    const int flags = cfg ? cfg->flags : 0;
    StreamLaunch r;
    const int rc = resolve_stream_launch({M, K, N, nnz, vec_limit(N, 16), variant, flags, kReduceSum, nullptr, cfg, false, nullptr}, &r);
    if (rc != 0 && rc != kNotStreaming) return rc;
    const Selection& sel = r.sel;
    const Geometry& g = sel.geo;
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
        const bool seg = r.segmented;
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
    return describe_result(n, capacity);
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
    int64_t nnz = -1, K = kMaxCols;
    gespmm_launch_cfg cfg = {0, 0, 0, 0, 0, 0};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (gespmm::auto_plan_enabled() && m > 0 && n > 0 && indptr && indices && B && C) {
        // (the fingerprint's read-back is the synchronisation this entry point performs anyway; K and nnz come out of it)
        int rc = 0;
        if (gespmm::auto_plan_try(indptr, indices, nullptr, B, C, m, 0, n, -1, GESPMM_VARIANT_AUTO, reduce, empty, stream, &rc)) return rc;
    }
    const bool capturing = stream_capture(st) != Capture::No;  // (a failed query counts as capturing; its error is cleared below)
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

// The four single-head SDDMM entry points: one body. elem: bytes per element of D1 / D2 — 4: fp32 (dtype is not looked at), 2: fp16 /
// bf16 operands, the dtype among the arguments that must make sense. `out` is fp32 either way. csr == false: rows are row ids, M is ignored.
static int sddmm_entry(const int32_t* rows, bool csr, const int32_t* colind, const void* D1, const void* D2, float* out, int elem, int dtype,
                       int64_t M, int64_t nnz, int64_t N, void* stream) {
    if (elem == 2 && !valid_x16_dtype(dtype)) return GESPMM_EINVAL;
    int rc = check_sddmm_sizes(csr, M, nnz, N);
    if (rc != 0) return rc;
    if (nnz == 0) return 0;
    rc = check_pointers({{rows, 4, true}, {colind, 4, true}, {out, 4, true}, {D1, elem, N > 0}, {D2, elem, N > 0}});
    if (rc != 0) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (elem == 2) return (int)launch_sddmm_x16(rows, csr, colind, D1, D2, out, dtype, csr ? M : 0, nnz, N, st);
    return (int)launch_sddmm(rows, csr, colind, static_cast<const float*>(D1), static_cast<const float*>(D2), out, csr ? M : 0, nnz, N, st);
}

int gespmm_sddmm_coo_f32(const int32_t* rowind, const int32_t* colind, const float* D1, const float* D2, float* out,
                         int64_t nnz, int64_t N, void* stream) {
    return sddmm_entry(rowind, false, colind, D1, D2, out, 4, 0, 0, nnz, N, stream);
}

int gespmm_sddmm_csr_f32(const int32_t* rowptr, const int32_t* colind, const float* D1, const float* D2, float* out,
                         int64_t M, int64_t nnz, int64_t N, void* stream) {
    return sddmm_entry(rowptr, true, colind, D1, D2, out, 4, 0, M, nnz, N, stream);
}

int gespmm_sddmm_coo_x16(const int32_t* rowind, const int32_t* colind, const void* D1, const void* D2, float* out, int dtype,
                         int64_t nnz, int64_t N, void* stream) {
    return sddmm_entry(rowind, false, colind, D1, D2, out, 2, dtype, 0, nnz, N, stream);
}

int gespmm_sddmm_csr_x16(const int32_t* rowptr, const int32_t* colind, const void* D1, const void* D2, float* out, int dtype,
                         int64_t M, int64_t nnz, int64_t N, void* stream) {
    return sddmm_entry(rowptr, true, colind, D1, D2, out, 2, dtype, M, nnz, N, stream);
}

static int describe_sddmm(int csr, int64_t M, int64_t nnz, int64_t N, int d1_align, int d2_align, int capturing, char* out,
                          int64_t capacity, int elem_size) {
    const int rc = check_sddmm_sizes(true, M, nnz, N);  // (M is looked at whatever the form)
    if (!out || capacity <= 0 || rc == GESPMM_EINVAL) return GESPMM_EINVAL;
    if (d1_align < elem_size || d2_align < elem_size || (d1_align & (d1_align - 1)) != 0 || (d2_align & (d2_align - 1)) != 0)
        return GESPMM_EINVAL;
    if (rc != 0) return rc;
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
    return describe_result(n, capacity);
}

int gespmm_describe_sddmm(int csr, int64_t M, int64_t nnz, int64_t N, int d1_align, int d2_align, int capturing, char* out,
                          int64_t capacity) {
    return describe_sddmm(csr, M, nnz, N, d1_align, d2_align, capturing, out, capacity, 4);
}

int gespmm_describe_sddmm_x16(int csr, int64_t M, int64_t nnz, int64_t N, int d1_align, int d2_align, int capturing, char* out,
                              int64_t capacity) {
    return describe_sddmm(csr, M, nnz, N, d1_align, d2_align, capturing, out, capacity, 2);
}

// The multi-head SDDMM (gespmm.h): D1 [., H F], D2 [., H F], out [nnz, H]. The checks of the single-head entries above, in their order.
// elem: bytes per element of D1 / D2 — 4: fp32 (dtype is not looked at), 2: fp16 / bf16, the dtype checked first (as sddmm_entry).
static int sddmm_heads_entry(const int32_t* rows, bool csr, const int32_t* colind, const void* D1, const void* D2, float* out, int elem,
                             int dtype, int64_t M, int64_t H, int64_t F, int64_t nnz, void* stream) {
    if (elem == 2 && !valid_x16_dtype(dtype)) return GESPMM_EINVAL;
    int rc = check_sddmm_heads_sizes(csr, M, H, F, nnz);
    if (rc != 0) return rc;
    if (nnz == 0) return 0;
    rc = check_pointers({{rows, 4, true}, {colind, 4, true}, {out, 4, true}, {D1, elem, F > 0}, {D2, elem, F > 0}});
    if (rc != 0) return rc;
    return run_sddmm_heads_elem(rows, csr, colind, D1, D2, out, elem == 2 ? dtype : 0, M, -1, H, F, nnz, stream);
}

int gespmm_sddmm_coo_heads_f32(const int32_t* rowind, const int32_t* colind, const float* D1, const float* D2, float* out, int64_t H,
                               int64_t F, int64_t nnz, void* stream) {
    return sddmm_heads_entry(rowind, false, colind, D1, D2, out, 4, 0, 0, H, F, nnz, stream);
}

int gespmm_sddmm_csr_heads_f32(const int32_t* rowptr, const int32_t* colind, const float* D1, const float* D2, float* out, int64_t M,
                               int64_t H, int64_t F, int64_t nnz, void* stream) {
    return sddmm_heads_entry(rowptr, true, colind, D1, D2, out, 4, 0, M, H, F, nnz, stream);
}

int gespmm_sddmm_coo_heads_x16(const int32_t* rowind, const int32_t* colind, const void* D1, const void* D2, float* out, int dtype, int64_t H,
                               int64_t F, int64_t nnz, void* stream) {
    return sddmm_heads_entry(rowind, false, colind, D1, D2, out, 2, dtype, 0, H, F, nnz, stream);
}

int gespmm_sddmm_csr_heads_x16(const int32_t* rowptr, const int32_t* colind, const void* D1, const void* D2, float* out, int dtype, int64_t M,
                               int64_t H, int64_t F, int64_t nnz, void* stream) {
    return sddmm_heads_entry(rowptr, true, colind, D1, D2, out, 2, dtype, M, H, F, nnz, stream);
}

static int describe_sddmm_heads(int csr, int64_t M, int64_t nnz, int64_t H, int64_t F, int d1_align, int d2_align, int capturing, char* out,
                                int64_t capacity, int elem_size) {
    if (!out || capacity <= 0) return GESPMM_EINVAL;
    if (d1_align < elem_size || d2_align < elem_size || (d1_align & (d1_align - 1)) != 0 || (d2_align & (d2_align - 1)) != 0) return GESPMM_EINVAL;
    const int rc = gespmm::check_sddmm_heads_sizes(csr != 0, M, H, F, nnz);
    if (rc != 0) return rc;
    int n;
    if (nnz == 0) {
        n = snprintf(out, (size_t)capacity, "form=none");
    } else if (F == 0) {
        n = snprintf(out, (size_t)capacity, "route=zeros");
    } else {
        const gespmm::SddmmHeadsLaunch r = gespmm::resolve_sddmm_heads(csr != 0, M, nnz, H, F, d1_align > 16 ? 16 : d1_align,
                                                                       d2_align > 16 ? 16 : d2_align, capturing != 0, gespmm::sddmm_heads_pin(),
                                                                       elem_size);
        if (r.route == gespmm::kSddmmHeadsPlain) {
            n = snprintf(out, (size_t)capacity, "route=plain ");
            if (n > 0 && n < capacity) {
                const int m = describe_sddmm(csr, M, nnz, F, d1_align, d2_align, capturing, out + n, capacity - n, elem_size);
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
    return describe_result(n, capacity);
}

int gespmm_describe_sddmm_heads(int csr, int64_t M, int64_t nnz, int64_t H, int64_t F, int d1_align, int d2_align, int capturing, char* out,
                                int64_t capacity) {
    return describe_sddmm_heads(csr, M, nnz, H, F, d1_align, d2_align, capturing, out, capacity, 4);
}

int gespmm_describe_sddmm_heads_x16(int csr, int64_t M, int64_t nnz, int64_t H, int64_t F, int d1_align, int d2_align, int capturing,
                                    char* out, int64_t capacity) {
    return describe_sddmm_heads(csr, M, nnz, H, F, d1_align, d2_align, capturing, out, capacity, 2);
}

/* The edge softmax over CSR rows (gespmm.h). One kernel for every size the checks let through; resolve_edge_softmax decides its shape. */
int gespmm_edge_softmax_f32(const int32_t* rowptr, const float* score, float* out, int64_t M, int64_t H, int64_t nnz, float slope,
                            void* stream) {
    const int rc = gespmm::check_edge_softmax_sizes(M, H, nnz, slope);
    if (rc != 0) return rc;
    if (nnz == 0) return 0;
    if (const int rcp = check_pointers({{rowptr, 4, true}, {score, 4, true}, {out, 4, true}})) return rcp;
    return (int)gespmm::launch_edge_softmax(rowptr, score, out, M, H, nnz, slope, gespmm::resolve_edge_softmax(M, nnz, H),
                                            reinterpret_cast<hipStream_t>(stream));
}

int gespmm_edge_softmax_backward_f32(const int32_t* rowptr, const float* alpha, const float* grad_alpha, const float* score,
                                     float* grad_score, int64_t M, int64_t H, int64_t nnz, float slope, void* stream) {
    const int rc = gespmm::check_edge_softmax_sizes(M, H, nnz, slope);
    if (rc != 0) return rc;
    if (nnz == 0) return 0;
    const bool leaky = slope != 1.0f;  // (score is looked at only then)
    if (const int rcp = check_pointers({{rowptr, 4, true}, {alpha, 4, true}, {grad_alpha, 4, true}, {grad_score, 4, true},
                                        {leaky ? score : nullptr, 4, leaky}}))
        return rcp;
    return (int)gespmm::launch_edge_softmax_backward(rowptr, alpha, grad_alpha, leaky ? score : nullptr, grad_score, M, H, nnz, slope,
                                                     gespmm::resolve_edge_softmax(M, nnz, H), reinterpret_cast<hipStream_t>(stream));
}

/* The same on the additive score el[row] + er[col] of a graph attention layer (gespmm.h): the score is a source trait of the one kernel. */
int gespmm_gat_softmax_f32(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, float* out, int64_t M, int64_t K,
                           int64_t H, int64_t nnz, float slope, void* stream) {
    const int rc = gespmm::check_gat_softmax_sizes(M, K, H, nnz, slope);
    if (rc != 0) return rc;
    if (nnz == 0) return 0;
    if (const int rcp = check_pointers({{rowptr, 4, true}, {colind, 4, true}, {el, 4, true}, {er, 4, true}, {out, 4, true}})) return rcp;
    return (int)gespmm::launch_gat_softmax(rowptr, colind, el, er, out, M, K, H, nnz, slope, gespmm::resolve_edge_softmax(M, nnz, H),
                                           reinterpret_cast<hipStream_t>(stream));
}

int gespmm_gat_softmax_backward_f32(const int32_t* rowptr, const int32_t* colind, const float* alpha, const float* grad_alpha,
                                    const float* el, const float* er, float* grad_score, float* grad_el, int64_t M, int64_t K, int64_t H,
                                    int64_t nnz, float slope, void* stream) {
    const int rc = gespmm::check_gat_softmax_sizes(M, K, H, nnz, slope);
    if (rc != 0) return rc;
    if (M == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const gespmm::EdgeSoftmaxLaunch r = gespmm::resolve_edge_softmax(M, nnz, H);
    if (nnz == 0) {  // every word of grad_el is still written
        if (const int rcp = check_pointers({{grad_el, 4, true}})) return rcp;
        return (int)gespmm::launch_gat_softmax_backward(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, grad_el, M, K, H, 0,
                                                        slope, r, st);
    }
    const bool leaky = slope != 1.0f;  // (the sign of el + er is looked at only then)
    if (const int rcp = check_pointers({{rowptr, 4, true}, {alpha, 4, true}, {grad_alpha, 4, true}, {grad_score, 4, true},
                                        {grad_el, 4, true}, {leaky ? colind : nullptr, 4, leaky}, {leaky ? el : nullptr, 4, leaky},
                                        {leaky ? er : nullptr, 4, leaky}}))
        return rcp;
    return (int)gespmm::launch_gat_softmax_backward(rowptr, leaky ? colind : nullptr, alpha, grad_alpha, leaky ? el : nullptr,
                                                    leaky ? er : nullptr, grad_score, grad_el, M, K, H, nnz, slope, r, st);
}

int gespmm_edge_segment_sum_f32(const int32_t* ptr, const int32_t* order, const float* x, float* out, int64_t S, int64_t H, int64_t nnz,
                                void* stream) {
    int rc = gespmm::check_edge_softmax_sizes(S, H, nnz, 1.0f);
    if (rc == 0) rc = gespmm::check_dense_words(S, H);
    if (rc != 0) return rc;
    if (S == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (nnz == 0) {  // every word of out is still written
        if (const int rcp = check_pointers({{out, 4, true}})) return rcp;
        return (int)gespmm::launch_edge_segment_sum(nullptr, nullptr, nullptr, out, S, H, 0, gespmm::resolve_edge_softmax(S, 0, H), st);
    }
    if (const int rcp = check_pointers({{ptr, 4, true}, {x, 4, true}, {out, 4, true}, {order, 4, false}})) return rcp;
    return (int)gespmm::launch_edge_segment_sum(ptr, order, x, out, S, H, nnz, gespmm::resolve_edge_softmax(S, nnz, H), st);
}

/* The row statistics of gespmm_gat_softmax_f32 (gespmm.h): the same kernel without the pass that writes alpha. */
int gespmm_gat_softmax_stats_f32(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, float* stats, int64_t M,
                                 int64_t K, int64_t H, int64_t nnz, float slope, void* stream) {
    const int rc = gespmm::check_gat_softmax_sizes(M, K, H, nnz, slope);
    if (rc != 0) return rc;
    if (M == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const gespmm::EdgeSoftmaxLaunch r = gespmm::resolve_edge_softmax(M, nnz, H);
    if (nnz == 0) {  // every word of stats is still written
        if (const int rcp = check_pointers({{stats, 8, true}})) return rcp;
        return (int)gespmm::launch_gat_softmax_stats(nullptr, nullptr, nullptr, nullptr, stats, M, K, H, 0, slope, r, st);
    }
    if (const int rcp = check_pointers({{rowptr, 4, true}, {colind, 4, true}, {el, 4, true}, {er, 4, true}, {stats, 8, true}})) return rcp;
    return (int)gespmm::launch_gat_softmax_stats(rowptr, colind, el, er, stats, M, K, H, nnz, slope, r, st);
}

/* The fused GAT aggregation (gespmm.h): one kernel that computes the weights where the multi-head product loads them, else the
   composition — the same weights into a stream-ordered temporary, then gespmm_csr_spmm_heads_f32 on it. Same bits either way. */
static int gat_aggregate_entry(const int32_t* ptr, const int32_t* ind, const float* el, const float* er, const float* stats, const float* B,
                               float* C, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, int transposed,
                               const float* p, const void* seed, void* stream) {
    if (transposed != 0 && transposed != 1) return GESPMM_EINVAL;
    int rc = gespmm::check_gat_aggregate_sizes(M, K, H, F, nnz, slope, transposed != 0);
    if (p) rc = gespmm::check_dropout_p(rc, *p);
    if (rc != 0) return rc;
    const int64_t S = transposed ? K : M, Kb = transposed ? M : K;  // segments, rows of B
    if (S == 0 || F == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (nnz == 0) {  // C = 0
        if (const int rcp = check_pointers({{C, 4, true}, {seed, 4, p != nullptr}})) return rcp;
        return (int)hipMemsetAsync(C, 0, (size_t)S * (size_t)H * (size_t)F * sizeof(float), st);
    }
    rc = check_pointers({{ptr, 4, true}, {ind, 4, true}, {el, 4, true}, {er, 4, true}, {stats, 8, true}, {B, 4, true}, {C, 4, true},
                         {seed, 4, p != nullptr}});
    if (rc != 0) return rc;
    const gespmm::GatTerms terms = {el, er, stats, slope};
    gespmm::EdgeDropout dropout = {};
    if (p) dropout = gespmm::make_edge_dropout(*p, seed);
    const gespmm::EdgeDropout* drop = p ? &dropout : nullptr;
    int kind = 0;
    rc = gespmm::run_gat_aggregate(csr_view(ptr, ind, nullptr, S, Kb, nnz, GESPMM_VARIANT_AUTO), terms, B, C, H, F, transposed != 0, stream,
                                   pointer_alignment(B), pointer_alignment(C), false, &kind, nullptr, drop);
    if (rc != kHeadsUnavailable) return rc;
    const size_t w_bytes = (size_t)nnz * (size_t)H * 4;
    PooledScratch scratch;
    if ((rc = scratch.open(w_bytes, st)) != 0) return rc;  // (nothing launched; a capturing stream: what the heads composition returns)
    float* w = scratch.take(w_bytes);
    rc = (int)gespmm::launch_gat_weights(ptr, ind, el, er, stats, w, S, H, nnz, slope, transposed != 0, st);
    if (rc == 0 && drop) rc = (int)gespmm::launch_edge_dropout(ptr, ind, w, w, S, H, nnz, *drop, transposed != 0, st);  // the same expression
    if (rc == 0) rc = gespmm_csr_spmm_heads_f32(ptr, ind, w, B, C, S, Kb, H, F, nnz, stream);
    return scratch.close(rc);
}

int gespmm_gat_aggregate_f32(const int32_t* ptr, const int32_t* ind, const float* el, const float* er, const float* stats, const float* B,
                             float* C, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, int transposed, void* stream) {
    return gat_aggregate_entry(ptr, ind, el, er, stats, B, C, M, K, H, F, nnz, slope, transposed, nullptr, nullptr, stream);
}

/* ... with dropout on the weights (gespmm.h; edge_dropout.h): the staged weight is dropout(weight), route 0 applies the same expression
   to its temporary. The ladder is the base entry's; a bad p joins the bad slope, the seed the pointers. */
int gespmm_gat_aggregate_dropout_f32(const int32_t* ptr, const int32_t* ind, const float* el, const float* er, const float* stats,
                                     const float* B, float* C, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope,
                                     int transposed, float p, const void* seed, void* stream) {
    return gat_aggregate_entry(ptr, ind, el, er, stats, B, C, M, K, H, F, nnz, slope, transposed, &p, seed, stream);
}

/* Dropout on an [nnz, H] array of the pattern (gespmm.h; edge_dropout.h): the softmax's ladder on (M, K, H, nnz) with p in the slope's
   place, then the pointers. */
int gespmm_edge_dropout_f32(const int32_t* rowptr, const int32_t* colind, const float* x, float* y, int64_t M, int64_t K, int64_t H,
                            int64_t nnz, float p, const void* seed, void* stream) {
    const int rc = gespmm::check_dropout_p(gespmm::check_gat_softmax_sizes(M, K, H, nnz, 1.0f), p);
    if (rc != 0) return rc;
    if (nnz == 0) return 0;
    if (const int rcp = check_pointers({{rowptr, 4, true}, {colind, 4, true}, {x, 4, true}, {y, 4, true}, {seed, 4, true}})) return rcp;
    return (int)gespmm::launch_edge_dropout(rowptr, colind, x, y, M, H, nnz, gespmm::make_edge_dropout(p, seed), false,
                                            reinterpret_cast<hipStream_t>(stream));
}

uint32_t gespmm_edge_dropout_bits(uint32_t s0, uint32_t s1, uint32_t r, uint32_t c, uint32_t h) {
    return gespmm::edge_dropout_bits(s0, s1, r, c, h);
}

/* T of edge_dropout.h for 0 <= p < 1. Anything else (NaN included) answers 0xffffffff, which no legal p gives (the largest float below 1
   gives 2^32 - 256). */
uint32_t gespmm_edge_dropout_threshold(float p) { return (p >= 0.0f && p < 1.0f) ? gespmm::edge_dropout_threshold(p) : 0xffffffffu; }

/* The fused backward of a GAT layer for el / er (gespmm.h; gat_backward.h): two launches on node-sized words, no [nnz x H] array. The
   ladder is check_gat_backward_sizes, then the pointers. */
static int gat_backward_el_entry(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, const float* stats,
                                 const float* grad_out, const float* feat, float* delta, float* grad_el, int64_t M, int64_t K, int64_t H,
                                 int64_t F, int64_t nnz, float slope, const float* p, const void* seed, void* stream) {
    int rc = gespmm::check_gat_backward_sizes(M, K, H, F, nnz, slope);
    if (p) rc = gespmm::check_dropout_p(rc, *p);
    if (rc != 0) return rc;
    if (M == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const gespmm::EdgeSoftmaxLaunch r = gespmm::resolve_edge_softmax(M, nnz, H);
    if (nnz == 0 || F == 0) {  // every g is an empty sum: every word of delta and grad_el is still written
        if (const int rcp = check_pointers({{delta, 4, true}, {grad_el, 4, true}, {seed, 4, p != nullptr}})) return rcp;
        return (int)gespmm::launch_gat_backward_el(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, delta, grad_el, M, K, H, F,
                                                   0, slope, r, nullptr, st);
    }
    if (const int rcp = check_pointers({{rowptr, 4, true}, {colind, 4, true}, {el, 4, true}, {er, 4, true}, {stats, 8, true},
                                        {grad_out, 4, true}, {feat, 4, true}, {delta, 4, true}, {grad_el, 4, true}, {seed, 4, p != nullptr}}))
        return rcp;
    gespmm::EdgeDropout dropout = {};
    if (p) dropout = gespmm::make_edge_dropout(*p, seed);
    return (int)gespmm::launch_gat_backward_el(rowptr, colind, el, er, stats, grad_out, feat, delta, grad_el, M, K, H, F, nnz, slope, r,
                                               p ? &dropout : nullptr, st);
}

int gespmm_gat_backward_el_f32(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, const float* stats,
                               const float* grad_out, const float* feat, float* delta, float* grad_el, int64_t M, int64_t K, int64_t H,
                               int64_t F, int64_t nnz, float slope, void* stream) {
    return gat_backward_el_entry(rowptr, colind, el, er, stats, grad_out, feat, delta, grad_el, M, K, H, F, nnz, slope, nullptr, nullptr, stream);
}

int gespmm_gat_backward_el_dropout_f32(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, const float* stats,
                                       const float* grad_out, const float* feat, float* delta, float* grad_el, int64_t M, int64_t K,
                                       int64_t H, int64_t F, int64_t nnz, float slope, float p, const void* seed, void* stream) {
    return gat_backward_el_entry(rowptr, colind, el, er, stats, grad_out, feat, delta, grad_el, M, K, H, F, nnz, slope, &p, seed, stream);
}

static int gat_backward_er_entry(const int32_t* colptr, const int32_t* rowind, const float* el, const float* er, const float* stats,
                                 const float* delta, const float* grad_out, const float* feat, float* grad_er, int64_t M, int64_t K, int64_t H,
                                 int64_t F, int64_t nnz, float slope, const float* p, const void* seed, void* stream) {
    int rc = gespmm::check_gat_backward_sizes(M, K, H, F, nnz, slope);
    if (p) rc = gespmm::check_dropout_p(rc, *p);
    if (rc != 0) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const gespmm::EdgeSoftmaxLaunch r = gespmm::resolve_edge_softmax(K, nnz, H);
    if (nnz == 0 || F == 0) {
        if (const int rcp = check_pointers({{grad_er, 4, true}, {seed, 4, p != nullptr}})) return rcp;
        return (int)gespmm::launch_gat_backward_er(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, grad_er, M, K, H, F,
                                                   0, slope, r, nullptr, st);
    }
    if (const int rcp = check_pointers({{colptr, 4, true}, {rowind, 4, true}, {el, 4, true}, {er, 4, true}, {stats, 8, true},
                                        {delta, 4, true}, {grad_out, 4, true}, {feat, 4, true}, {grad_er, 4, true}, {seed, 4, p != nullptr}}))
        return rcp;
    gespmm::EdgeDropout dropout = {};
    if (p) dropout = gespmm::make_edge_dropout(*p, seed);
    return (int)gespmm::launch_gat_backward_er(colptr, rowind, el, er, stats, delta, grad_out, feat, grad_er, M, K, H, F, nnz, slope, r,
                                               p ? &dropout : nullptr, st);
}

int gespmm_gat_backward_er_f32(const int32_t* colptr, const int32_t* rowind, const float* el, const float* er, const float* stats,
                               const float* delta, const float* grad_out, const float* feat, float* grad_er, int64_t M, int64_t K, int64_t H,
                               int64_t F, int64_t nnz, float slope, void* stream) {
    return gat_backward_er_entry(colptr, rowind, el, er, stats, delta, grad_out, feat, grad_er, M, K, H, F, nnz, slope, nullptr, nullptr, stream);
}

int gespmm_gat_backward_er_dropout_f32(const int32_t* colptr, const int32_t* rowind, const float* el, const float* er, const float* stats,
                                       const float* delta, const float* grad_out, const float* feat, float* grad_er, int64_t M, int64_t K,
                                       int64_t H, int64_t F, int64_t nnz, float slope, float p, const void* seed, void* stream) {
    return gat_backward_er_entry(colptr, rowind, el, er, stats, delta, grad_out, feat, grad_er, M, K, H, F, nnz, slope, &p, seed, stream);
}

int gespmm_gat_aggregate_route(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, int transposed, int b_align, int c_align,
                               int32_t* geometry_out) {
    if (b_align < 1 || c_align < 1 || (transposed != 0 && transposed != 1)) return GESPMM_EINVAL;
    const int rc0 = gespmm::check_gat_aggregate_sizes(M, K, H, F, nnz, 1.0f, transposed != 0);
    if (rc0 != 0) return rc0;
    const int64_t S = transposed ? K : M, Kb = transposed ? M : K;
    int kind = 0;
    Geometry geo = {};
    const gespmm::GatTerms none = {nullptr, nullptr, nullptr, 1.0f};
    const int rc = gespmm::run_gat_aggregate(csr_view(nullptr, nullptr, nullptr, S, Kb, nnz, GESPMM_VARIANT_AUTO), none, nullptr, nullptr, H, F,
                                             transposed != 0, nullptr, b_align, c_align, true, &kind, &geo);
    const int route = route_result(rc == kHeadsUnavailable ? 0 : rc, kind);
    if (route >= 0 && geometry_out) {
        geometry_out[0] = kind ? geo.vec : 0;
        geometry_out[1] = kind ? geo.strips : 0;
        geometry_out[2] = kind ? geo.group : 0;
        geometry_out[3] = kind ? geo.rows_per_wave : 0;
    }
    return route;
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
    return describe_result(n, capacity);
}

/* The GATv2 edge score and its gradients (gespmm.h; gatv2_score.h): one kernel each, nothing larger than [nnz x H]. */
int gespmm_gatv2_score_f32(const int32_t* rowptr, const int32_t* colind, const float* xl, const float* xr, const float* att, float* score,
                           int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, void* stream) {
    const int rc = gespmm::check_gatv2_sizes(M, K, H, F, nnz, slope);
    if (rc != 0) return rc;
    if (nnz == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (F == 0) {
        if (const int rcp = check_pointers({{score, 4, true}})) return rcp;
        return (int)hipMemsetAsync(score, 0, (size_t)nnz * (size_t)H * sizeof(float), st);
    }
    if (const int rcp = check_pointers({{rowptr, 4, true}, {colind, 4, true}, {xl, 4, true}, {xr, 4, true}, {att, 4, true}, {score, 4, true}}))
        return rcp;
    const gespmm::Gatv2ScoreLaunch r =
        gespmm::resolve_gatv2_score(M, nnz, H, F, pointer_alignment(xl), pointer_alignment(xr), pointer_alignment(att));
    return (int)gespmm::launch_gatv2_score(rowptr, colind, xl, xr, att, score, M, nnz, H, F, slope, r, st);
}

int gespmm_gatv2_score_backward_f32(const int32_t* ptr, const int32_t* ind, const int32_t* order, const float* grad_score,
                                    const float* x_seg, const float* x_ind, const float* att, float* grad_x, float* att_part, int64_t S,
                                    int64_t T, int64_t H, int64_t F, int64_t nnz, float slope, void* stream) {
    const int rc = gespmm::check_gatv2_sizes(S, T, H, F, nnz, slope);
    if (rc != 0) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (nnz == 0 || F == 0) {  // every chain is empty: every word of the results is still written
        if (const int rcp = check_pointers({{grad_x, 4, true}, {att_part, 4, false}})) return rcp;
        const size_t bytes = (size_t)S * (size_t)H * (size_t)F * sizeof(float);
        if (bytes == 0) return 0;
        hipError_t e = hipMemsetAsync(grad_x, 0, bytes, st);
        if (e == hipSuccess && att_part) e = hipMemsetAsync(att_part, 0, bytes, st);
        return (int)e;
    }
    if (const int rcp = check_pointers({{ptr, 4, true}, {ind, 4, true}, {grad_score, 4, true}, {x_seg, 4, true}, {x_ind, 4, true},
                                        {att, 4, true}, {grad_x, 4, true}, {order, 4, false}, {att_part, 4, false}}))
        return rcp;
    int align = 16;
    for (const void* p : {(const void*)x_seg, (const void*)x_ind, (const void*)att, (const void*)grad_x, (const void*)att_part})
        if (p) align = std::min(align, pointer_alignment(p));
    return (int)gespmm::launch_gatv2_score_backward(ptr, ind, order, grad_score, x_seg, x_ind, att, grad_x, att_part, S, H, F, nnz, slope,
                                                    vec_limit(F, align) == 4, st);
}

int gespmm_describe_gatv2_score(int64_t M, int64_t nnz, int64_t H, int64_t F, int xl_align, int xr_align, int att_align, char* out,
                                int64_t capacity) {
    if (!out || capacity <= 0) return GESPMM_EINVAL;
    for (const int a : {xl_align, xr_align, att_align})
        if (a < 4 || (a & (a - 1)) != 0) return GESPMM_EINVAL;
    const int rc = gespmm::check_gatv2_sizes(M, nnz > 0 ? 1 : 0, H, F, nnz, 1.0f);  // (the forward's launch shape does not depend on K)
    if (rc != 0) return rc;
    int n;
    if (nnz == 0) {
        n = snprintf(out, (size_t)capacity, "form=none");
    } else if (F == 0) {
        n = snprintf(out, (size_t)capacity, "route=zeros");
    } else {
        const gespmm::Gatv2ScoreLaunch r = gespmm::resolve_gatv2_score(M, nnz, H, F, xl_align > 16 ? 16 : xl_align,
                                                                       xr_align > 16 ? 16 : xr_align, att_align > 16 ? 16 : att_align);
        n = snprintf(out, (size_t)capacity, "V=%d W=%d epw=%d", r.V, r.W, r.epw);
    }
    return describe_result(n, capacity);
}

/* ... on fp16 / bf16 node operands (gespmm.h; gatv2_score.h): the dtype code first, as in every _x16 entry, then the ladders above with
   2-byte alignment for the 16-bit operands. */
int gespmm_gatv2_score_x16(const int32_t* rowptr, const int32_t* colind, const void* xl, const void* xr, const float* att, float* score,
                           int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, void* stream) {
    if (!gespmm::valid_x16_dtype(dtype)) return GESPMM_EINVAL;
    const int rc = gespmm::check_gatv2_sizes(M, K, H, F, nnz, slope);
    if (rc != 0) return rc;
    if (nnz == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (F == 0) {
        if (const int rcp = check_pointers({{score, 4, true}})) return rcp;
        return (int)hipMemsetAsync(score, 0, (size_t)nnz * (size_t)H * sizeof(float), st);
    }
    if (const int rcp = check_pointers({{rowptr, 4, true}, {colind, 4, true}, {xl, 2, true}, {xr, 2, true}, {att, 4, true}, {score, 4, true}}))
        return rcp;
    const gespmm::Gatv2ScoreLaunch r =
        gespmm::resolve_gatv2_score_x16(M, nnz, H, F, pointer_alignment(xl), pointer_alignment(xr), pointer_alignment(att));
    return (int)gespmm::launch_gatv2_score_x16(rowptr, colind, xl, xr, att, score, dtype, M, nnz, H, F, slope, r, st);
}

int gespmm_gatv2_score_backward_x16(const int32_t* ptr, const int32_t* ind, const int32_t* order, const float* grad_score,
                                    const void* x_seg, const void* x_ind, const float* att, void* grad_x, float* att_part, int dtype,
                                    int64_t S, int64_t T, int64_t H, int64_t F, int64_t nnz, float slope, void* stream) {
    if (!gespmm::valid_x16_dtype(dtype)) return GESPMM_EINVAL;
    const int rc = gespmm::check_gatv2_sizes(S, T, H, F, nnz, slope);
    if (rc != 0) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (nnz == 0 || F == 0) {  // every chain is empty: every word of the results is still written (+0 has no set bit in either type)
        if (const int rcp = check_pointers({{grad_x, 2, true}, {att_part, 4, false}})) return rcp;
        const size_t elems = (size_t)S * (size_t)H * (size_t)F;
        if (elems == 0) return 0;
        hipError_t e = hipMemsetAsync(grad_x, 0, elems * sizeof(uint16_t), st);
        if (e == hipSuccess && att_part) e = hipMemsetAsync(att_part, 0, elems * sizeof(float), st);
        return (int)e;
    }
    if (const int rcp = check_pointers({{ptr, 4, true}, {ind, 4, true}, {grad_score, 4, true}, {x_seg, 2, true}, {x_ind, 2, true},
                                        {att, 4, true}, {grad_x, 2, true}, {order, 4, false}, {att_part, 4, false}}))
        return rcp;
    int f_align = pointer_alignment(att);
    if (att_part) f_align = std::min(f_align, pointer_alignment(att_part));
    const int x_align = gespmm::least_alignment({x_seg, x_ind, grad_x});
    return (int)gespmm::launch_gatv2_score_backward_x16(ptr, ind, order, grad_score, x_seg, x_ind, att, grad_x, att_part, dtype, S, H, F, nnz,
                                                        slope, gespmm::gatv2_score_x16_vec(F, x_align, std::min(f_align, 16)), st);
}

int gespmm_describe_gatv2_score_x16(int64_t M, int64_t nnz, int64_t H, int64_t F, int xl_align, int xr_align, int att_align, char* out,
                                    int64_t capacity) {
    if (!out || capacity <= 0) return GESPMM_EINVAL;
    for (const int a : {xl_align, xr_align, att_align})
        if (a < 2 || (a & (a - 1)) != 0) return GESPMM_EINVAL;
    if (att_align < 4) return GESPMM_EINVAL;
    const int rc = gespmm::check_gatv2_sizes(M, nnz > 0 ? 1 : 0, H, F, nnz, 1.0f);  // (the forward's launch shape does not depend on K)
    if (rc != 0) return rc;
    int n;
    if (nnz == 0) {
        n = snprintf(out, (size_t)capacity, "form=none");
    } else if (F == 0) {
        n = snprintf(out, (size_t)capacity, "route=zeros");
    } else {
        const gespmm::Gatv2ScoreLaunch r = gespmm::resolve_gatv2_score_x16(M, nnz, H, F, xl_align > 16 ? 16 : xl_align,
                                                                           xr_align > 16 ? 16 : xr_align, att_align > 16 ? 16 : att_align);
        n = snprintf(out, (size_t)capacity, "V=%d W=%d epw=%d", r.V, r.W, r.epw);
    }
    return describe_result(n, capacity);
}

/* Fused scaled dot-product attention over a pattern and its backward (gespmm.h; dot_attention.h): one kernel each, nothing of size nnz
   but the index arrays. The ladder is check_dot_attention_sizes, nnz == 0, F == 0, then the pointers. */
static int zero_fill(std::initializer_list<std::pair<float*, size_t>> outs, hipStream_t st) {
    for (const auto& o : outs)
        if (!o.first && o.second) return GESPMM_EINVAL;
    for (const auto& o : outs)
        if (reinterpret_cast<uintptr_t>(o.first) % 4 != 0) return GESPMM_EALIGN;
    for (const auto& o : outs) {
        if (o.second == 0) continue;
        const hipError_t e = hipMemsetAsync(o.first, 0, o.second * sizeof(float), st);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

static int dot_attention_entry(const int32_t* rowptr, const int32_t* colind, const float* q, const float* k, const float* v, float* out,
                               float* stats, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, const float* p,
                               const void* seed, void* stream) {
    const int rc = gespmm::check_dot_attention_sizes(M, K, H, F, nnz, scale, p);
    if (rc != 0) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (nnz == 0 || F == 0) {  // every row is empty (F == 0: there is nothing to attend with): every word of the results is still written
        if (const int rcp = check_pointers({{seed, 4, p != nullptr}})) return rcp;
        return zero_fill({{out, (size_t)(M * H * F)}, {stats, (size_t)(M * H * 2)}}, st);
    }
    if (const int rcp = check_pointers({{rowptr, 4, true}, {colind, 4, true}, {q, 4, true}, {k, 4, true}, {v, 4, true}, {out, 4, true},
                                        {stats, 8, true}, {seed, 4, p != nullptr}}))
        return rcp;
    const int a = gespmm::least_alignment({q, k, v, out});
    gespmm::EdgeDropout dropout = {};
    if (p) dropout = gespmm::make_edge_dropout(*p, seed);
    return (int)gespmm::launch_dot_attention(rowptr, colind, q, k, v, out, stats, M, K, H, F, nnz, scale,
                                             gespmm::resolve_dot_attention(F, a, a, a), p ? &dropout : nullptr, st);
}

int gespmm_dot_attention_f32(const int32_t* rowptr, const int32_t* colind, const float* q, const float* k, const float* v, float* out,
                             float* stats, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, void* stream) {
    return dot_attention_entry(rowptr, colind, q, k, v, out, stats, M, K, H, F, nnz, scale, nullptr, nullptr, stream);
}

int gespmm_dot_attention_dropout_f32(const int32_t* rowptr, const int32_t* colind, const float* q, const float* k, const float* v, float* out,
                                     float* stats, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, float p,
                                     const void* seed, void* stream) {
    return dot_attention_entry(rowptr, colind, q, k, v, out, stats, M, K, H, F, nnz, scale, &p, seed, stream);
}

static int dot_attention_backward_q_entry(const int32_t* rowptr, const int32_t* colind, const float* q, const float* k, const float* v,
                                          const float* stats, const float* out, const float* grad_out, float* delta, float* grad_q,
                                          int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, const float* p,
                                          const void* seed, void* stream) {
    const int rc = gespmm::check_dot_attention_sizes(M, K, H, F, nnz, scale, p);
    if (rc != 0) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (nnz == 0 || F == 0) {
        if (const int rcp = check_pointers({{seed, 4, p != nullptr}})) return rcp;
        return zero_fill({{delta, (size_t)(M * H)}, {grad_q, (size_t)(M * H * F)}}, st);
    }
    if (const int rcp = check_pointers({{rowptr, 4, true}, {colind, 4, true}, {q, 4, true}, {k, 4, true}, {v, 4, true}, {stats, 8, true},
                                        {out, 4, true}, {grad_out, 4, true}, {delta, 4, true}, {grad_q, 4, true}, {seed, 4, p != nullptr}}))
        return rcp;
    const int a = gespmm::least_alignment({q, k, v, out, grad_out, grad_q});
    gespmm::EdgeDropout dropout = {};
    if (p) dropout = gespmm::make_edge_dropout(*p, seed);
    return (int)gespmm::launch_dot_attention_backward_q(rowptr, colind, q, k, v, stats, out, grad_out, delta, grad_q, M, K, H, F, nnz, scale,
                                                        gespmm::resolve_dot_attention(F, a, a, a), p ? &dropout : nullptr, st);
}

int gespmm_dot_attention_backward_q_f32(const int32_t* rowptr, const int32_t* colind, const float* q, const float* k, const float* v,
                                        const float* stats, const float* out, const float* grad_out, float* delta, float* grad_q, int64_t M,
                                        int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, void* stream) {
    return dot_attention_backward_q_entry(rowptr, colind, q, k, v, stats, out, grad_out, delta, grad_q, M, K, H, F, nnz, scale, nullptr, nullptr,
                                          stream);
}

int gespmm_dot_attention_backward_q_dropout_f32(const int32_t* rowptr, const int32_t* colind, const float* q, const float* k, const float* v,
                                                const float* stats, const float* out, const float* grad_out, float* delta, float* grad_q,
                                                int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, float p, const void* seed,
                                                void* stream) {
    return dot_attention_backward_q_entry(rowptr, colind, q, k, v, stats, out, grad_out, delta, grad_q, M, K, H, F, nnz, scale, &p, seed, stream);
}

static int dot_attention_backward_kv_entry(const int32_t* colptr, const int32_t* rowind, const float* q, const float* k, const float* v,
                                           const float* stats, const float* delta, const float* grad_out, float* grad_k, float* grad_v,
                                           int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, const float* p,
                                           const void* seed, void* stream) {
    const int rc = gespmm::check_dot_attention_sizes(M, K, H, F, nnz, scale, p);
    if (rc != 0) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (nnz == 0 || F == 0) {
        if (const int rcp = check_pointers({{seed, 4, p != nullptr}})) return rcp;
        return zero_fill({{grad_k, (size_t)(K * H * F)}, {grad_v, (size_t)(K * H * F)}}, st);
    }
    if (const int rcp = check_pointers({{colptr, 4, true}, {rowind, 4, true}, {q, 4, true}, {k, 4, true}, {v, 4, true}, {stats, 8, true},
                                        {delta, 4, true}, {grad_out, 4, true}, {grad_k, 4, true}, {grad_v, 4, true}, {seed, 4, p != nullptr}}))
        return rcp;
    const int a = gespmm::least_alignment({q, k, v, grad_out, grad_k, grad_v});
    gespmm::EdgeDropout dropout = {};
    if (p) dropout = gespmm::make_edge_dropout(*p, seed);
    return (int)gespmm::launch_dot_attention_backward_kv(colptr, rowind, q, k, v, stats, delta, grad_out, grad_k, grad_v, M, K, H, F, nnz,
                                                         scale, gespmm::resolve_dot_attention(F, a, a, a), p ? &dropout : nullptr, st);
}

int gespmm_dot_attention_backward_kv_f32(const int32_t* colptr, const int32_t* rowind, const float* q, const float* k, const float* v,
                                         const float* stats, const float* delta, const float* grad_out, float* grad_k, float* grad_v,
                                         int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, void* stream) {
    return dot_attention_backward_kv_entry(colptr, rowind, q, k, v, stats, delta, grad_out, grad_k, grad_v, M, K, H, F, nnz, scale, nullptr,
                                           nullptr, stream);
}

int gespmm_dot_attention_backward_kv_dropout_f32(const int32_t* colptr, const int32_t* rowind, const float* q, const float* k, const float* v,
                                                 const float* stats, const float* delta, const float* grad_out, float* grad_k, float* grad_v,
                                                 int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, float p,
                                                 const void* seed, void* stream) {
    return dot_attention_backward_kv_entry(colptr, rowind, q, k, v, stats, delta, grad_out, grad_k, grad_v, M, K, H, F, nnz, scale, &p, seed,
                                           stream);
}

int gespmm_describe_dot_attention(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, int q_align, int k_align, int v_align, char* out,
                                  int64_t capacity) {
    if (!out || capacity <= 0) return GESPMM_EINVAL;
    for (const int a : {q_align, k_align, v_align})
        if (a < 4 || (a & (a - 1)) != 0) return GESPMM_EINVAL;
    const int rc = gespmm::check_dot_attention_sizes(M, K, H, F, nnz, 1.0f, nullptr);
    if (rc != 0 && rc != GESPMM_ERR_UNSUPPORTED) return rc;
    int n;
    if (rc == GESPMM_ERR_UNSUPPORTED) {
        n = snprintf(out, (size_t)capacity, "route=unsupported");
    } else if (nnz == 0) {
        n = snprintf(out, (size_t)capacity, "form=none");
    } else if (F == 0) {
        n = snprintf(out, (size_t)capacity, "route=zeros");
    } else {
        const gespmm::DotAttentionLaunch r =
            gespmm::resolve_dot_attention(F, q_align > 16 ? 16 : q_align, k_align > 16 ? 16 : k_align, v_align > 16 ? 16 : v_align);
        n = snprintf(out, (size_t)capacity, "V=%d W=%d", r.V, r.W);
    }
    return describe_result(n, capacity);
}

/* Fused GATv2 attention over a pattern and its backward (gespmm.h; gatv2_attention.h): one kernel each, nothing of size nnz but the
   index arrays. The ladder is check_gatv2_attention_sizes, nnz == 0, F == 0, then the pointers — that of the dot-product attention. */
static int gatv2_attention_entry(const int32_t* rowptr, const int32_t* colind, const float* xl, const float* xr, const float* att, float* out,
                                 float* stats, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, const float* p,
                                 const void* seed, void* stream) {
    const int rc = gespmm::check_gatv2_attention_sizes(M, K, H, F, nnz, slope, p);
    if (rc != 0) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (nnz == 0 || F == 0) {  // every row is empty (F == 0: there is nothing to attend with): every word of the results is still written
        if (const int rcp = check_pointers({{seed, 4, p != nullptr}})) return rcp;
        return zero_fill({{out, (size_t)(M * H * F)}, {stats, (size_t)(M * H * 2)}}, st);
    }
    if (const int rcp = check_pointers({{rowptr, 4, true}, {colind, 4, true}, {xl, 4, true}, {xr, 4, true}, {att, 4, true}, {out, 4, true},
                                        {stats, 8, true}, {seed, 4, p != nullptr}}))
        return rcp;
    const int a = gespmm::least_alignment({xl, xr, att, out});
    gespmm::EdgeDropout dropout = {};
    if (p) dropout = gespmm::make_edge_dropout(*p, seed);
    return (int)gespmm::launch_gatv2_attention(rowptr, colind, xl, xr, att, out, stats, M, K, H, F, nnz, slope,
                                               gespmm::resolve_gatv2_attention(F, a, a, a), p ? &dropout : nullptr, st);
}

int gespmm_gatv2_attention_f32(const int32_t* rowptr, const int32_t* colind, const float* xl, const float* xr, const float* att, float* out,
                               float* stats, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, void* stream) {
    return gatv2_attention_entry(rowptr, colind, xl, xr, att, out, stats, M, K, H, F, nnz, slope, nullptr, nullptr, stream);
}

int gespmm_gatv2_attention_dropout_f32(const int32_t* rowptr, const int32_t* colind, const float* xl, const float* xr, const float* att,
                                       float* out, float* stats, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope,
                                       float p, const void* seed, void* stream) {
    return gatv2_attention_entry(rowptr, colind, xl, xr, att, out, stats, M, K, H, F, nnz, slope, &p, seed, stream);
}

static int gatv2_attention_backward_row_entry(const int32_t* rowptr, const int32_t* colind, const float* xl, const float* xr,
                                              const float* att, const float* stats, const float* out, const float* grad_out, float* delta,
                                              float* grad_xl, float* att_part, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz,
                                              float slope, const float* p, const void* seed, void* stream) {
    const int rc = gespmm::check_gatv2_attention_sizes(M, K, H, F, nnz, slope, p);
    if (rc != 0) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (nnz == 0 || F == 0) {
        if (const int rcp = check_pointers({{seed, 4, p != nullptr}})) return rcp;
        return zero_fill({{delta, (size_t)(M * H)}, {grad_xl, (size_t)(M * H * F)}, {att_part, att_part ? (size_t)(M * H * F) : 0}}, st);
    }
    if (const int rcp = check_pointers({{rowptr, 4, true}, {colind, 4, true}, {xl, 4, true}, {xr, 4, true}, {att, 4, true}, {stats, 8, true},
                                        {out, 4, true}, {grad_out, 4, true}, {delta, 4, true}, {grad_xl, 4, true}, {att_part, 4, false},
                                        {seed, 4, p != nullptr}}))
        return rcp;
    const int a = gespmm::least_alignment({xl, xr, att, out, grad_out, grad_xl, att_part});  // (a null att_part counts as aligned)
    gespmm::EdgeDropout dropout = {};
    if (p) dropout = gespmm::make_edge_dropout(*p, seed);
    return (int)gespmm::launch_gatv2_attention_backward_row(rowptr, colind, xl, xr, att, stats, out, grad_out, delta, grad_xl, att_part, M, K,
                                                            H, F, nnz, slope, gespmm::resolve_gatv2_attention(F, a, a, a),
                                                            p ? &dropout : nullptr, st);
}

int gespmm_gatv2_attention_backward_row_f32(const int32_t* rowptr, const int32_t* colind, const float* xl, const float* xr, const float* att,
                                            const float* stats, const float* out, const float* grad_out, float* delta, float* grad_xl,
                                            float* att_part, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope,
                                            void* stream) {
    return gatv2_attention_backward_row_entry(rowptr, colind, xl, xr, att, stats, out, grad_out, delta, grad_xl, att_part, M, K, H, F, nnz,
                                              slope, nullptr, nullptr, stream);
}

int gespmm_gatv2_attention_backward_row_dropout_f32(const int32_t* rowptr, const int32_t* colind, const float* xl, const float* xr,
                                                    const float* att, const float* stats, const float* out, const float* grad_out,
                                                    float* delta, float* grad_xl, float* att_part, int64_t M, int64_t K, int64_t H,
                                                    int64_t F, int64_t nnz, float slope, float p, const void* seed, void* stream) {
    return gatv2_attention_backward_row_entry(rowptr, colind, xl, xr, att, stats, out, grad_out, delta, grad_xl, att_part, M, K, H, F, nnz,
                                              slope, &p, seed, stream);
}

static int gatv2_attention_backward_col_entry(const int32_t* colptr, const int32_t* rowind, const float* xl, const float* xr,
                                              const float* att, const float* stats, const float* delta, const float* grad_out,
                                              float* grad_xr, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope,
                                              const float* p, const void* seed, void* stream) {
    const int rc = gespmm::check_gatv2_attention_sizes(M, K, H, F, nnz, slope, p);
    if (rc != 0) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (nnz == 0 || F == 0) {
        if (const int rcp = check_pointers({{seed, 4, p != nullptr}})) return rcp;
        return zero_fill({{grad_xr, (size_t)(K * H * F)}}, st);
    }
    if (const int rcp = check_pointers({{colptr, 4, true}, {rowind, 4, true}, {xl, 4, true}, {xr, 4, true}, {att, 4, true}, {stats, 8, true},
                                        {delta, 4, true}, {grad_out, 4, true}, {grad_xr, 4, true}, {seed, 4, p != nullptr}}))
        return rcp;
    const int a = gespmm::least_alignment({xl, xr, att, grad_out, grad_xr});
    gespmm::EdgeDropout dropout = {};
    if (p) dropout = gespmm::make_edge_dropout(*p, seed);
    return (int)gespmm::launch_gatv2_attention_backward_col(colptr, rowind, xl, xr, att, stats, delta, grad_out, grad_xr, M, K, H, F, nnz,
                                                            slope, gespmm::resolve_gatv2_attention(F, a, a, a), p ? &dropout : nullptr, st);
}

int gespmm_gatv2_attention_backward_col_f32(const int32_t* colptr, const int32_t* rowind, const float* xl, const float* xr, const float* att,
                                            const float* stats, const float* delta, const float* grad_out, float* grad_xr, int64_t M,
                                            int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, void* stream) {
    return gatv2_attention_backward_col_entry(colptr, rowind, xl, xr, att, stats, delta, grad_out, grad_xr, M, K, H, F, nnz, slope, nullptr,
                                              nullptr, stream);
}

int gespmm_gatv2_attention_backward_col_dropout_f32(const int32_t* colptr, const int32_t* rowind, const float* xl, const float* xr,
                                                    const float* att, const float* stats, const float* delta, const float* grad_out,
                                                    float* grad_xr, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope,
                                                    float p, const void* seed, void* stream) {
    return gatv2_attention_backward_col_entry(colptr, rowind, xl, xr, att, stats, delta, grad_out, grad_xr, M, K, H, F, nnz, slope, &p, seed,
                                              stream);
}

int gespmm_describe_gatv2_attention(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, int xl_align, int xr_align, int att_align,
                                    char* out, int64_t capacity) {
    if (!out || capacity <= 0) return GESPMM_EINVAL;
    for (const int a : {xl_align, xr_align, att_align})
        if (a < 4 || (a & (a - 1)) != 0) return GESPMM_EINVAL;
    const int rc = gespmm::check_gatv2_attention_sizes(M, K, H, F, nnz, 1.0f, nullptr);
    if (rc != 0 && rc != GESPMM_ERR_UNSUPPORTED) return rc;
    int n;
    if (rc == GESPMM_ERR_UNSUPPORTED) {
        n = snprintf(out, (size_t)capacity, "route=unsupported supported=0");
    } else if (nnz == 0) {
        n = snprintf(out, (size_t)capacity, "form=none supported=1");
    } else if (F == 0) {
        n = snprintf(out, (size_t)capacity, "route=zeros supported=1");
    } else {
        const gespmm::Gatv2AttentionLaunch r = gespmm::resolve_gatv2_attention(F, xl_align > 16 ? 16 : xl_align,
                                                                               xr_align > 16 ? 16 : xr_align, att_align > 16 ? 16 : att_align);
        n = snprintf(out, (size_t)capacity, "V=%d W=%d supported=%d", r.V, r.W, r.supported ? 1 : 0);
    }
    return describe_result(n, capacity);
}

/* ... on fp16 / bf16 node terms (gespmm.h; gatv2_attention_x16.h): the dtype code first, as in every _x16 entry, then the ladder above
   with 2-byte alignment for the 16-bit operands and results. att, stats, delta and att_part stay fp32. */
struct ZeroFillArg {
    void* p;
    int elem;      // bytes
    size_t count;  // elements; 0: the array is absent or empty
};
static int zero_fill_x16(std::initializer_list<ZeroFillArg> outs, hipStream_t st) {
    for (const auto& o : outs)
        if (!o.p && o.count) return GESPMM_EINVAL;
    for (const auto& o : outs)
        if (reinterpret_cast<uintptr_t>(o.p) % (uintptr_t)o.elem != 0) return GESPMM_EALIGN;
    for (const auto& o : outs) {
        if (o.count == 0) continue;
        const hipError_t e = hipMemsetAsync(o.p, 0, o.count * (size_t)o.elem, st);  // (+0 has no set bit in either type)
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

static int gatv2_attention_x16_entry(const int32_t* rowptr, const int32_t* colind, const void* xl, const void* xr, const float* att, void* out,
                                     float* stats, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope,
                                     const float* p, const void* seed, void* stream) {
    if (!gespmm::valid_x16_dtype(dtype)) return GESPMM_EINVAL;
    const int rc = gespmm::check_gatv2_attention_sizes(M, K, H, F, nnz, slope, p);
    if (rc != 0) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (nnz == 0 || F == 0) {  // every row is empty: every word of the results is still written
        if (const int rcp = check_pointers({{seed, 4, p != nullptr}})) return rcp;
        return zero_fill_x16({{out, 2, (size_t)(M * H * F)}, {stats, 4, (size_t)(M * H * 2)}}, st);
    }
    if (const int rcp = check_pointers({{rowptr, 4, true}, {colind, 4, true}, {xl, 2, true}, {xr, 2, true}, {att, 4, true}, {out, 2, true},
                                        {stats, 8, true}, {seed, 4, p != nullptr}}))
        return rcp;
    const int a = gespmm::least_alignment({xl, xr, out});
    gespmm::EdgeDropout dropout = {};
    if (p) dropout = gespmm::make_edge_dropout(*p, seed);
    return (int)gespmm::launch_gatv2_attention_x16(rowptr, colind, xl, xr, att, out, stats, dtype, M, K, H, F, nnz, slope,
                                                   gespmm::resolve_gatv2_attention_x16(F, a, a, pointer_alignment(att)),
                                                   p ? &dropout : nullptr, st);
}

int gespmm_gatv2_attention_x16(const int32_t* rowptr, const int32_t* colind, const void* xl, const void* xr, const float* att, void* out,
                               float* stats, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, void* stream) {
    return gatv2_attention_x16_entry(rowptr, colind, xl, xr, att, out, stats, dtype, M, K, H, F, nnz, slope, nullptr, nullptr, stream);
}

int gespmm_gatv2_attention_dropout_x16(const int32_t* rowptr, const int32_t* colind, const void* xl, const void* xr, const float* att,
                                       void* out, float* stats, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz,
                                       float slope, float p, const void* seed, void* stream) {
    return gatv2_attention_x16_entry(rowptr, colind, xl, xr, att, out, stats, dtype, M, K, H, F, nnz, slope, &p, seed, stream);
}

static int gatv2_attention_backward_row_x16_entry(const int32_t* rowptr, const int32_t* colind, const void* xl, const void* xr,
                                                  const float* att, const float* stats, const void* out, const void* grad_out, float* delta,
                                                  void* grad_xl, float* att_part, int dtype, int64_t M, int64_t K, int64_t H, int64_t F,
                                                  int64_t nnz, float slope, const float* p, const void* seed, void* stream) {
    if (!gespmm::valid_x16_dtype(dtype)) return GESPMM_EINVAL;
    const int rc = gespmm::check_gatv2_attention_sizes(M, K, H, F, nnz, slope, p);
    if (rc != 0) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (nnz == 0 || F == 0) {
        if (const int rcp = check_pointers({{seed, 4, p != nullptr}})) return rcp;
        return zero_fill_x16({{delta, 4, (size_t)(M * H)}, {grad_xl, 2, (size_t)(M * H * F)},
                              {att_part, 4, att_part ? (size_t)(M * H * F) : 0}}, st);
    }
    if (const int rcp = check_pointers({{rowptr, 4, true}, {colind, 4, true}, {xl, 2, true}, {xr, 2, true}, {att, 4, true}, {stats, 8, true},
                                        {out, 2, true}, {grad_out, 2, true}, {delta, 4, true}, {grad_xl, 2, true}, {att_part, 4, false},
                                        {seed, 4, p != nullptr}}))
        return rcp;
    const int a = gespmm::least_alignment({xl, xr, out, grad_out, grad_xl});
    const int fa = gespmm::least_alignment({att, att_part});  // (a null att_part counts as aligned)
    gespmm::EdgeDropout dropout = {};
    if (p) dropout = gespmm::make_edge_dropout(*p, seed);
    return (int)gespmm::launch_gatv2_attention_backward_row_x16(rowptr, colind, xl, xr, att, stats, out, grad_out, delta, grad_xl, att_part,
                                                                dtype, M, K, H, F, nnz, slope,
                                                                gespmm::resolve_gatv2_attention_x16(F, a, a, fa), p ? &dropout : nullptr, st);
}

int gespmm_gatv2_attention_backward_row_x16(const int32_t* rowptr, const int32_t* colind, const void* xl, const void* xr, const float* att,
                                            const float* stats, const void* out, const void* grad_out, float* delta, void* grad_xl,
                                            float* att_part, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope,
                                            void* stream) {
    return gatv2_attention_backward_row_x16_entry(rowptr, colind, xl, xr, att, stats, out, grad_out, delta, grad_xl, att_part, dtype, M, K, H,
                                                  F, nnz, slope, nullptr, nullptr, stream);
}

int gespmm_gatv2_attention_backward_row_dropout_x16(const int32_t* rowptr, const int32_t* colind, const void* xl, const void* xr,
                                                    const float* att, const float* stats, const void* out, const void* grad_out,
                                                    float* delta, void* grad_xl, float* att_part, int dtype, int64_t M, int64_t K, int64_t H,
                                                    int64_t F, int64_t nnz, float slope, float p, const void* seed, void* stream) {
    return gatv2_attention_backward_row_x16_entry(rowptr, colind, xl, xr, att, stats, out, grad_out, delta, grad_xl, att_part, dtype, M, K, H,
                                                  F, nnz, slope, &p, seed, stream);
}

static int gatv2_attention_backward_col_x16_entry(const int32_t* colptr, const int32_t* rowind, const void* xl, const void* xr,
                                                  const float* att, const float* stats, const float* delta, const void* grad_out,
                                                  void* grad_xr, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz,
                                                  float slope, const float* p, const void* seed, void* stream) {
    if (!gespmm::valid_x16_dtype(dtype)) return GESPMM_EINVAL;
    const int rc = gespmm::check_gatv2_attention_sizes(M, K, H, F, nnz, slope, p);
    if (rc != 0) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (nnz == 0 || F == 0) {
        if (const int rcp = check_pointers({{seed, 4, p != nullptr}})) return rcp;
        return zero_fill_x16({{grad_xr, 2, (size_t)(K * H * F)}}, st);
    }
    if (const int rcp = check_pointers({{colptr, 4, true}, {rowind, 4, true}, {xl, 2, true}, {xr, 2, true}, {att, 4, true}, {stats, 8, true},
                                        {delta, 4, true}, {grad_out, 2, true}, {grad_xr, 2, true}, {seed, 4, p != nullptr}}))
        return rcp;
    const int a = gespmm::least_alignment({xl, xr, grad_out, grad_xr});
    gespmm::EdgeDropout dropout = {};
    if (p) dropout = gespmm::make_edge_dropout(*p, seed);
    return (int)gespmm::launch_gatv2_attention_backward_col_x16(colptr, rowind, xl, xr, att, stats, delta, grad_out, grad_xr, dtype, M, K, H, F,
                                                                nnz, slope,
                                                                gespmm::resolve_gatv2_attention_x16(F, a, a, pointer_alignment(att)),
                                                                p ? &dropout : nullptr, st);
}

int gespmm_gatv2_attention_backward_col_x16(const int32_t* colptr, const int32_t* rowind, const void* xl, const void* xr, const float* att,
                                            const float* stats, const float* delta, const void* grad_out, void* grad_xr, int dtype, int64_t M,
                                            int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, void* stream) {
    return gatv2_attention_backward_col_x16_entry(colptr, rowind, xl, xr, att, stats, delta, grad_out, grad_xr, dtype, M, K, H, F, nnz, slope,
                                                  nullptr, nullptr, stream);
}

int gespmm_gatv2_attention_backward_col_dropout_x16(const int32_t* colptr, const int32_t* rowind, const void* xl, const void* xr,
                                                    const float* att, const float* stats, const float* delta, const void* grad_out,
                                                    void* grad_xr, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz,
                                                    float slope, float p, const void* seed, void* stream) {
    return gatv2_attention_backward_col_x16_entry(colptr, rowind, xl, xr, att, stats, delta, grad_out, grad_xr, dtype, M, K, H, F, nnz, slope,
                                                  &p, seed, stream);
}

int gespmm_describe_gatv2_attention_x16(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, int xl_align, int xr_align, int att_align,
                                        char* out, int64_t capacity) {
    if (!out || capacity <= 0) return GESPMM_EINVAL;
    for (const int a : {xl_align, xr_align, att_align})
        if (a < 2 || (a & (a - 1)) != 0) return GESPMM_EINVAL;
    if (att_align < 4) return GESPMM_EINVAL;
    const int rc = gespmm::check_gatv2_attention_sizes(M, K, H, F, nnz, 1.0f, nullptr);
    if (rc != 0 && rc != GESPMM_ERR_UNSUPPORTED) return rc;
    int n;
    if (rc == GESPMM_ERR_UNSUPPORTED) {
        n = snprintf(out, (size_t)capacity, "route=unsupported supported=0");
    } else if (nnz == 0) {
        n = snprintf(out, (size_t)capacity, "form=none supported=1");
    } else if (F == 0) {
        n = snprintf(out, (size_t)capacity, "route=zeros supported=1");
    } else {
        const gespmm::Gatv2AttentionLaunch r = gespmm::resolve_gatv2_attention_x16(
            F, xl_align > 16 ? 16 : xl_align, xr_align > 16 ? 16 : xr_align, att_align > 16 ? 16 : att_align);
        n = snprintf(out, (size_t)capacity, "V=%d W=%d supported=%d", r.V, r.W, r.supported ? 1 : 0);
    }
    return describe_result(n, capacity);
}

/* The fused dot-product attention on fp16 / bf16 q, k and v (gespmm.h; dot_attention_x16.h): the dtype code first, as in every _x16
   entry, then the ladder of the _f32 entries with 2-byte alignment for the 16-bit operands and results. stats and delta stay fp32. */
static int dot_attention_x16_entry(const int32_t* rowptr, const int32_t* colind, const void* q, const void* k, const void* v, void* out,
                                   float* stats, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale,
                                   const float* p, const void* seed, void* stream) {
    if (!gespmm::valid_x16_dtype(dtype)) return GESPMM_EINVAL;
    const int rc = gespmm::check_dot_attention_sizes(M, K, H, F, nnz, scale, p);
    if (rc != 0) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (nnz == 0 || F == 0) {  // every row is empty: every word of the results is still written
        if (const int rcp = check_pointers({{seed, 4, p != nullptr}})) return rcp;
        return zero_fill_x16({{out, 2, (size_t)(M * H * F)}, {stats, 4, (size_t)(M * H * 2)}}, st);
    }
    if (const int rcp = check_pointers({{rowptr, 4, true}, {colind, 4, true}, {q, 2, true}, {k, 2, true}, {v, 2, true}, {out, 2, true},
                                        {stats, 8, true}, {seed, 4, p != nullptr}}))
        return rcp;
    const int a = gespmm::least_alignment({q, k, v, out});
    gespmm::EdgeDropout dropout = {};
    if (p) dropout = gespmm::make_edge_dropout(*p, seed);
    return (int)gespmm::launch_dot_attention_x16(rowptr, colind, q, k, v, out, stats, dtype, M, K, H, F, nnz, scale,
                                                 gespmm::resolve_dot_attention_x16(F, a, a, a), p ? &dropout : nullptr, st);
}

int gespmm_dot_attention_x16(const int32_t* rowptr, const int32_t* colind, const void* q, const void* k, const void* v, void* out,
                             float* stats, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, void* stream) {
    return dot_attention_x16_entry(rowptr, colind, q, k, v, out, stats, dtype, M, K, H, F, nnz, scale, nullptr, nullptr, stream);
}

int gespmm_dot_attention_dropout_x16(const int32_t* rowptr, const int32_t* colind, const void* q, const void* k, const void* v, void* out,
                                     float* stats, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, float p,
                                     const void* seed, void* stream) {
    return dot_attention_x16_entry(rowptr, colind, q, k, v, out, stats, dtype, M, K, H, F, nnz, scale, &p, seed, stream);
}

static int dot_attention_backward_q_x16_entry(const int32_t* rowptr, const int32_t* colind, const void* q, const void* k, const void* v,
                                              const float* stats, const void* out, const void* grad_out, float* delta, void* grad_q,
                                              int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale,
                                              const float* p, const void* seed, void* stream) {
    if (!gespmm::valid_x16_dtype(dtype)) return GESPMM_EINVAL;
    const int rc = gespmm::check_dot_attention_sizes(M, K, H, F, nnz, scale, p);
    if (rc != 0) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (nnz == 0 || F == 0) {
        if (const int rcp = check_pointers({{seed, 4, p != nullptr}})) return rcp;
        return zero_fill_x16({{delta, 4, (size_t)(M * H)}, {grad_q, 2, (size_t)(M * H * F)}}, st);
    }
    if (const int rcp = check_pointers({{rowptr, 4, true}, {colind, 4, true}, {q, 2, true}, {k, 2, true}, {v, 2, true}, {stats, 8, true},
                                        {out, 2, true}, {grad_out, 2, true}, {delta, 4, true}, {grad_q, 2, true}, {seed, 4, p != nullptr}}))
        return rcp;
    const int a = gespmm::least_alignment({q, k, v, out, grad_out, grad_q});
    gespmm::EdgeDropout dropout = {};
    if (p) dropout = gespmm::make_edge_dropout(*p, seed);
    return (int)gespmm::launch_dot_attention_backward_q_x16(rowptr, colind, q, k, v, stats, out, grad_out, delta, grad_q, dtype, M, K, H, F,
                                                            nnz, scale, gespmm::resolve_dot_attention_x16(F, a, a, a),
                                                            p ? &dropout : nullptr, st);
}

int gespmm_dot_attention_backward_q_x16(const int32_t* rowptr, const int32_t* colind, const void* q, const void* k, const void* v,
                                        const float* stats, const void* out, const void* grad_out, float* delta, void* grad_q, int dtype,
                                        int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, void* stream) {
    return dot_attention_backward_q_x16_entry(rowptr, colind, q, k, v, stats, out, grad_out, delta, grad_q, dtype, M, K, H, F, nnz, scale,
                                              nullptr, nullptr, stream);
}

int gespmm_dot_attention_backward_q_dropout_x16(const int32_t* rowptr, const int32_t* colind, const void* q, const void* k, const void* v,
                                                const float* stats, const void* out, const void* grad_out, float* delta, void* grad_q,
                                                int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, float p,
                                                const void* seed, void* stream) {
    return dot_attention_backward_q_x16_entry(rowptr, colind, q, k, v, stats, out, grad_out, delta, grad_q, dtype, M, K, H, F, nnz, scale, &p,
                                              seed, stream);
}

static int dot_attention_backward_kv_x16_entry(const int32_t* colptr, const int32_t* rowind, const void* q, const void* k, const void* v,
                                               const float* stats, const float* delta, const void* grad_out, void* grad_k, void* grad_v,
                                               int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale,
                                               const float* p, const void* seed, void* stream) {
    if (!gespmm::valid_x16_dtype(dtype)) return GESPMM_EINVAL;
    const int rc = gespmm::check_dot_attention_sizes(M, K, H, F, nnz, scale, p);
    if (rc != 0) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (nnz == 0 || F == 0) {
        if (const int rcp = check_pointers({{seed, 4, p != nullptr}})) return rcp;
        return zero_fill_x16({{grad_k, 2, (size_t)(K * H * F)}, {grad_v, 2, (size_t)(K * H * F)}}, st);
    }
    if (const int rcp = check_pointers({{colptr, 4, true}, {rowind, 4, true}, {q, 2, true}, {k, 2, true}, {v, 2, true}, {stats, 8, true},
                                        {delta, 4, true}, {grad_out, 2, true}, {grad_k, 2, true}, {grad_v, 2, true}, {seed, 4, p != nullptr}}))
        return rcp;
    const int a = gespmm::least_alignment({q, k, v, grad_out, grad_k, grad_v});
    gespmm::EdgeDropout dropout = {};
    if (p) dropout = gespmm::make_edge_dropout(*p, seed);
    return (int)gespmm::launch_dot_attention_backward_kv_x16(colptr, rowind, q, k, v, stats, delta, grad_out, grad_k, grad_v, dtype, M, K, H,
                                                             F, nnz, scale, gespmm::resolve_dot_attention_x16(F, a, a, a),
                                                             p ? &dropout : nullptr, st);
}

int gespmm_dot_attention_backward_kv_x16(const int32_t* colptr, const int32_t* rowind, const void* q, const void* k, const void* v,
                                         const float* stats, const float* delta, const void* grad_out, void* grad_k, void* grad_v, int dtype,
                                         int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, void* stream) {
    return dot_attention_backward_kv_x16_entry(colptr, rowind, q, k, v, stats, delta, grad_out, grad_k, grad_v, dtype, M, K, H, F, nnz, scale,
                                               nullptr, nullptr, stream);
}

int gespmm_dot_attention_backward_kv_dropout_x16(const int32_t* colptr, const int32_t* rowind, const void* q, const void* k, const void* v,
                                                 const float* stats, const float* delta, const void* grad_out, void* grad_k, void* grad_v,
                                                 int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, float p,
                                                 const void* seed, void* stream) {
    return dot_attention_backward_kv_x16_entry(colptr, rowind, q, k, v, stats, delta, grad_out, grad_k, grad_v, dtype, M, K, H, F, nnz, scale,
                                               &p, seed, stream);
}

int gespmm_describe_dot_attention_x16(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, int q_align, int k_align, int v_align,
                                      char* out, int64_t capacity) {
    if (!out || capacity <= 0) return GESPMM_EINVAL;
    for (const int a : {q_align, k_align, v_align})
        if (a < 2 || (a & (a - 1)) != 0) return GESPMM_EINVAL;
    const int rc = gespmm::check_dot_attention_sizes(M, K, H, F, nnz, 1.0f, nullptr);
    if (rc != 0 && rc != GESPMM_ERR_UNSUPPORTED) return rc;
    int n;
    if (rc == GESPMM_ERR_UNSUPPORTED) {
        n = snprintf(out, (size_t)capacity, "route=unsupported");
    } else if (nnz == 0) {
        n = snprintf(out, (size_t)capacity, "form=none");
    } else if (F == 0) {
        n = snprintf(out, (size_t)capacity, "route=zeros");
    } else {
        const gespmm::DotAttentionLaunch r =
            gespmm::resolve_dot_attention_x16(F, q_align > 16 ? 16 : q_align, k_align > 16 ? 16 : k_align, v_align > 16 ? 16 : v_align);
        n = snprintf(out, (size_t)capacity, "V=%d W=%d", r.V, r.W);
    }
    return describe_result(n, capacity);
}

int gespmm_baseline_atomic_scatter_f32(const int32_t* rowptr, const int32_t* colind, const float* in, float* out,
                                       int64_t M, int64_t K, int64_t N, int64_t nnz, void* stream) {
    if (M < 0 || K < 0 || N < 0 || nnz < 0) return GESPMM_EINVAL;
    if (M > kSddmmMaxRows || K > kMaxCols || N > kMaxWidth || nnz > kInt32Max) return GESPMM_ERANGE;
    if (K == 0 || N == 0) return 0;
    if (!out || (nnz > 0 && (!rowptr || !colind || !in))) return GESPMM_EINVAL;
    return (int)gespmm::launch_atomic_scatter(rowptr, colind, in, out, M, K, N, nnz,
                                              reinterpret_cast<hipStream_t>(stream));
}

int gespmm_baseline_copy_f32(const float* src, float* dst, int64_t n, void* stream) {
    if (n < 0) return GESPMM_EINVAL;
    if (n == 0) return 0;
    if (const int rc = check_pointers({{src, 4, true}, {dst, 4, true}})) return rc;
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
    if (M > kSddmmMaxRows || K > kInt32Max - 1 || nnz > kInt32Max) return GESPMM_ERANGE;
    if (!rowptr || !colptr) return GESPMM_EINVAL;
    if (nnz > 0 && (!colind || !rowind || !workspace)) return GESPMM_EINVAL;
    if ((csr_val == nullptr) != (csc_val == nullptr)) return GESPMM_EINVAL;
    return (int)gespmm::launch_csr2csc(rowptr, colind, csr_val, colptr, rowind, csc_val, M, K, nnz, workspace,
                                       reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
