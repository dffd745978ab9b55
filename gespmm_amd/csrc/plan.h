// plan.h — internal interface between the C ABI (capi.cpp) and the plan object (plan.cpp).
#pragma once
#include <stdint.h>

#include <initializer_list>

#include "../../include/gespmm.h"
#include "select.h"
#include "spmm_kernels.h"

namespace gespmm {

struct PlanLaunch {
    const int32_t* tasks;  // int4 per task (device)
    int32_t ntasks;
    const int32_t* perm;   // permuted row -> original row (device)
    const int32_t* gtasks; // int4 per lane-group task of the segmented-stream kernel (device), may be NULL
    int32_t ngtasks;
    bool prefer_segmented; // launch the segmented-stream kernel when the geometry allows it
};

// The matrix a product launches on: the caller's CSR arrays, or a plan's row-clustered copy with its task tables (plan.cpp: plan_view
// builds it from the plan and its route). A dry run looks at the sizes, the variant and the tables only.
struct CsrView {
    const int32_t* rowptr;
    const int32_t* colind;
    const float* val;  // NULL: A == 1 on its pattern (the multi-head product: [nnz, H], with tables in the plan's entry order)
    int64_t M, K, nnz;
    int variant;
    bool planned;      // `pl` holds a plan's task tables
    PlanLaunch pl;
    const PlanLaunch* tables() const { return planned ? &pl : nullptr; }
};
inline CsrView csr_view(const int32_t* rowptr, const int32_t* colind, const float* val, int64_t M, int64_t K, int64_t nnz, int variant) {
    return {rowptr, colind, val, M, K, nnz, variant, false, {}};
}

// ---- what every entry point checks its arguments with. Order, everywhere: sizes that make no sense (GESPMM_EINVAL), sizes that do not
// fit (GESPMM_ERANGE), nothing to do (the entry point's own return), required pointers that are NULL (GESPMM_EINVAL), alignment (GESPMM_EALIGN).
constexpr int64_t kInt32Max = 0x7fffffffLL;
constexpr int64_t kMaxRows = kInt32Max - 64;      // M of the products: CSR positions are int32 and the kernels look up to a few tiles past a row's end before clamping
constexpr int64_t kMaxCols = kInt32Max;           // K
constexpr int64_t kMaxWidth = kInt32Max / 4;      // N (H F of the multi-head calls): the bytes of a dense row
constexpr int64_t kMaxNnz = kInt32Max - 4096;     // entries of the products (the margin of kSddmmMaxNnz, spmm_kernels.h)
constexpr int64_t kSddmmMaxRows = kInt32Max - 1;  // M of the SDDMM family
inline bool valid_variant(int variant) { return variant >= GESPMM_VARIANT_AUTO && variant < GESPMM_NUM_VARIANTS; }
inline bool valid_x16_dtype(int dtype) { return dtype == GESPMM_X16_F16 || dtype == GESPMM_X16_BF16; }
// CSR x dense sizes (N: the width): GESPMM_EINVAL / GESPMM_ERANGE / 0. min_nnz: -1 where the entry point takes "not known".
int check_csr_sizes(int64_t M, int64_t K, int64_t N, int64_t nnz, int64_t min_nnz);
// SDDMM sizes: csr == false ignores M.
int check_sddmm_sizes(bool csr, int64_t M, int64_t nnz, int64_t N);
// GESPMM_EINVAL where a required pointer is NULL, then GESPMM_EALIGN where one (NULL counts as aligned) is not a multiple of its element size
struct PointerArg {
    const void* p;
    int elem;       // bytes
    bool required;
};
int check_pointers(std::initializer_list<PointerArg> args);
int check_heads_sizes(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz);              // GESPMM_EINVAL / GESPMM_ERANGE / 0: sizes alone
int check_sddmm_heads_sizes(bool csr, int64_t M, int64_t H, int64_t F, int64_t nnz);         // as above; csr == false ignores M and bounds nnz H
int pointer_alignment(const void* p);  // largest power of two (<= 16) that divides the address
// The V limit of a streaming launch: the widest vector (1, 2, 4 floats) that divides `unit` floats and that operands on `align`-byte boundaries can be addressed with
int vec_limit(int64_t unit, int align);
inline int min_alignment(const void* a, const void* b) { return pointer_alignment(a) < pointer_alignment(b) ? pointer_alignment(a) : pointer_alignment(b); }
// the last lines of every describe function (n: what snprintf returned) and of every dry-route query (rc: the dry call's, route: its answer)
inline int describe_result(int n, int64_t capacity) { return n < 0 ? GESPMM_EINVAL : n < capacity ? n : (int)capacity - 1; }
inline int route_result(int rc, int route) { return rc != 0 ? (rc < 0 ? rc : GESPMM_EINVAL) : route; }

// ---- is the stream capturing? One query (capi.cpp), three answers: what a failed query means is the caller's business.
enum class Capture { No, Yes, QueryFailed };
Capture stream_capture(hipStream_t st);  // leaves a failed query's error for the caller to clear, or not
bool is_capturing(hipStream_t st);       // a failed query counts as "no"; its error is cleared
// hipErrorStreamCaptureUnsupported when `st` is capturing (a composition that would have to allocate launches nothing), else 0
int refuse_allocation_under_capture(hipStream_t st);

// ---- one streaming launch, resolved: which of the two streaming kernels, in which lane geometry, with which flags.
struct StreamQuery {
    int64_t M, K, N, nnz;           // N: the width the selector sees
    int max_vec;                    // vec_limit of the product
    int variant, flags, reduce;
    const PlanLaunch* tables;       // a plan's task tables: the plan rule (no cache blocking, the kernel the tables are for, CRC family)
    const gespmm_launch_cfg* knobs; // vec / strips / group / rows_per_wave / slab_rows (NULL: none); its flags are NOT read
    bool ask_stream;                // the capture rule: on a capturing `stream` only the paths that allocate nothing
    hipStream_t stream;
};
struct StreamLaunch {
    Selection sel;
    int flags;       // the query's, after the capture rule and the plan rule
    bool segmented;  // the segmented-stream kernel (else batch-stream) — where the selection is a streaming kernel at all
    int rpw;         // rows per lane group / per wavefront of that kernel
};
constexpr int kNotStreaming = -104;  // internal: the selection is the naive or the parallel-reduction variant (*out is filled in)
// 0, kNotStreaming or what resolve_geometry refused the query with
int resolve_stream_launch(const StreamQuery& q, StreamLaunch* out);

// The one place every SpMM entry point ends up in (plan.cpp included: A carries the plan's task tables).
int run_spmm(const CsrView& A, const float* B, float* C, int64_t N, const gespmm_launch_cfg* cfg, int reduce, float empty, void* stream,
             void* ws, int64_t ws_bytes, const LaunchGuard* guard = nullptr);
// The fused product (gespmm_csr_spmm_fused_f32 / gespmm_plan_spmm_fused_f32) as ONE launch of a fused streaming kernel, where the unfused
// launch of the same arguments would be one streaming kernel (no long-row pass, no cache blocking, 32-bit offsets, a geometry the fused
// kernels are built for — spmm_fused.h). *kind: 1 batch-stream, 2 segmented-stream, 0 not available (kFusedUnavailable is returned and
// nothing is launched: the caller composes the product from the unfused launch). dry_run: answer only — pointers are not looked at,
// operands count as 16-byte aligned. `flags`: GESPMM_FLAG_* as in gespmm_launch_cfg.flags (a plan's launch_flags).
struct FusedVectors {
    const float* col_scale;
    const float* row_scale;
    const float* bias;
    bool any() const { return col_scale || row_scale || bias; }
};
constexpr int kFusedUnavailable = -101;  // internal
int run_spmm_fused(const CsrView& A, const float* B, const FusedVectors& fx, float* C, int64_t N, int flags, void* stream, bool dry_run,
                   int* kind);

// 16-bit dense operands (gespmm_csr_spmm_x16 / gespmm_plan_spmm_x16) as ONE launch of a 16-bit streaming kernel, where the fp32 launch of
// the byte-equivalent width N / 2 would be one streaming kernel in a geometry the 16-bit kernels are built for (spmm_x16.h), N is even
// and B and C are 4-byte aligned. *kind: 1 batch-stream, 2 segmented-stream, 0 not available (kX16Unavailable is returned and nothing is
// launched: the caller composes widen, the fp32 route, narrow). b_align / c_align: powers of two that divide the operands' addresses;
// dry_run: answer only — pointers are not looked at, and whether the stream is capturing is not asked.
constexpr int kX16Unavailable = -102;  // internal
int run_spmm_x16(const CsrView& A, const void* B, void* C, int dtype, int64_t N, int flags, void* stream, int b_align, int c_align,
                 bool dry_run, int* kind, Geometry* geo_out = nullptr);  // geo_out: the lane geometry (in words) of the kernel *kind names

// The multi-head product (gespmm_csr_spmm_heads_f32 / gespmm_plan_spmm_heads_f32; spmm_heads.h) as ONE launch of the heads kernel: 2 <= H <=
// kHeadsMax, 32-bit offsets (K H F 4 < 2^32, nnz H < 2^31) and a batch-stream geometry the kernel is built for, resolved for width H F with V
// limited to what divides F and what b_align / c_align allow, strict order, no cache blocking. *kind: 1 the kernel, 0 not available
// (kHeadsUnavailable is returned and nothing is launched: the caller composes per head). dry_run: answer only, pointers are not looked at.
constexpr int kHeadsUnavailable = -103;  // internal
// order (may be NULL; storage order only): the weights of entry p are row order[p] of A.val — the ordered kernels (spmm_heads_order.hip).
int run_spmm_heads(const CsrView& A, const float* B, float* C, int64_t H, int64_t F, int flags, void* stream, int b_align, int c_align,
                   bool dry_run, int* kind, Geometry* geo_out = nullptr, const int32_t* order = nullptr);

// The multi-head SDDMM (gespmm_sddmm_{coo,csr}_heads_f32 / gespmm_plan_sddmm_heads_f32; sddmm_heads.h) on checked arguments with nnz > 0:
// the route resolve_sddmm_heads answers (select.h). rows: row pointers (csr) or row ids. K: rows of D2 where the caller knows them, else
// -1 — only the CSR composition needs them and then finds a bound on the device (one stream synchronisation).
int run_sddmm_heads(const int32_t* rows, bool csr, const int32_t* colind, const float* D1, const float* D2, float* out, int64_t M, int64_t K,
                    int64_t H, int64_t F, int64_t nnz, void* stream);

// A plan's product behind a launch guard (auto_plan.cpp): kNotGuardable — and nothing launched — when the plan's launch is more than
// one kernel (hub rows handed to the long-row pass, the cache-blocked path).
int plan_spmm_guarded(gespmm_plan* plan, const float* B, float* C, int64_t N, int reduce, float empty, void* stream, const LaunchGuard* guard);

}  // namespace gespmm
