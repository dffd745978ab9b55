// plan.h — internal interface between the C ABI (capi.cpp) and the plan object (plan.cpp).
#pragma once
#include <stdint.h>

#include "../../include/gespmm.h"
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

int run_spmm(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B, float* C, int64_t M,
             int64_t K, int64_t N, int64_t nnz, int variant, const gespmm_launch_cfg* cfg, int reduce, float empty,
             void* stream, void* ws, int64_t ws_bytes, const PlanLaunch* pl, const LaunchGuard* guard = nullptr);
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
int run_spmm_fused(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B, const FusedVectors& fx, float* C,
                   int64_t M, int64_t K, int64_t N, int64_t nnz, int variant, int flags, void* stream, const PlanLaunch* pl, bool dry_run,
                   int* kind);
// argument checks of the fused entry points (no device work): sizes, NULLs, 4-byte alignment of every pointer
int check_fused_args(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B, const FusedVectors& fx, const float* C,
                     int64_t M, int64_t K, int64_t N, int64_t nnz);
// hipErrorStreamCaptureUnsupported when `st` is capturing (a composition that would have to allocate launches nothing), else 0
int refuse_allocation_under_capture(hipStream_t st);

// 16-bit dense operands (gespmm_csr_spmm_x16 / gespmm_plan_spmm_x16) as ONE launch of a 16-bit streaming kernel, where the fp32 launch of
// the byte-equivalent width N / 2 would be one streaming kernel in a geometry the 16-bit kernels are built for (spmm_x16.h), N is even
// and B and C are 4-byte aligned. *kind: 1 batch-stream, 2 segmented-stream, 0 not available (kX16Unavailable is returned and nothing is
// launched: the caller composes widen, the fp32 route, narrow). b_align / c_align: powers of two that divide the operands' addresses;
// dry_run: answer only — pointers are not looked at, and whether the stream is capturing is not asked.
constexpr int kX16Unavailable = -102;  // internal
int run_spmm_x16(const int32_t* rowptr, const int32_t* colind, const float* val, const void* B, void* C, int dtype, int64_t M, int64_t K,
                 int64_t N, int64_t nnz, int variant, int flags, void* stream, const PlanLaunch* pl, int b_align, int c_align, bool dry_run,
                 int* kind, Geometry* geo_out = nullptr);  // geo_out: the lane geometry (in words) of the kernel *kind names
int check_x16_args(const int32_t* rowptr, const int32_t* colind, const float* val, const void* B, const void* C, int dtype, int64_t M,
                   int64_t K, int64_t N, int64_t nnz);
int pointer_alignment(const void* p);  // largest power of two (<= 16) that divides the address

// The multi-head product (gespmm_csr_spmm_heads_f32 / gespmm_plan_spmm_heads_f32; spmm_heads.h) as ONE launch of the heads kernel: 2 <= H <=
// kHeadsMax, 32-bit offsets (K H F 4 < 2^32, nnz H < 2^31) and a batch-stream geometry the kernel is built for, resolved for width H F with V
// limited to what divides F and what b_align / c_align allow, strict order, no cache blocking. *kind: 1 the kernel, 0 not available
// (kHeadsUnavailable is returned and nothing is launched: the caller composes per head). `val` is [nnz, H] — with `pl` in the plan's entry
// order. dry_run: answer only, pointers are not looked at.
constexpr int kHeadsUnavailable = -103;  // internal
int run_spmm_heads(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B, float* C, int64_t M, int64_t K, int64_t H,
                   int64_t F, int64_t nnz, int variant, int flags, void* stream, const PlanLaunch* pl, int b_align, int c_align, bool dry_run,
                   int* kind, Geometry* geo_out = nullptr);
int check_heads_sizes(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz);  // GESPMM_EINVAL / GESPMM_ERANGE / 0: sizes alone
int check_heads_args(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B, const float* C, int64_t M, int64_t K,
                     int64_t H, int64_t F, int64_t nnz);

// The multi-head SDDMM (gespmm_sddmm_{coo,csr}_heads_f32 / gespmm_plan_sddmm_heads_f32; sddmm_heads.h) on checked arguments with nnz > 0:
// the route resolve_sddmm_heads answers (select.h). rows: row pointers (csr) or row ids. K: rows of D2 where the caller knows them, else
// -1 — only the CSR composition needs them and then finds a bound on the device (one stream synchronisation).
int run_sddmm_heads(const int32_t* rows, bool csr, const int32_t* colind, const float* D1, const float* D2, float* out, int64_t M, int64_t K,
                    int64_t H, int64_t F, int64_t nnz, void* stream);
int check_sddmm_heads_sizes(bool csr, int64_t M, int64_t H, int64_t F, int64_t nnz);  // GESPMM_EINVAL / GESPMM_ERANGE / 0: sizes alone

// A plan's product behind a launch guard (auto_plan.cpp): kNotGuardable — and nothing launched — when the plan's launch is more than
// one kernel (hub rows handed to the long-row pass, the cache-blocked path).
int plan_spmm_guarded(gespmm_plan* plan, const float* B, float* C, int64_t N, int reduce, float empty, void* stream, const LaunchGuard* guard);

}  // namespace gespmm
