// plan.cpp — gespmm_plan: the "analysis" stage in front of repeated SpMM calls on ONE sparse matrix.
//
// The reference launches its kernels straight on the caller's CSR (spmmWrapper, spmm_test.cu:456-492;
// spmm_cuda, pytorch-custom/spmm_kernel.cu:425-458) and has no such stage; vendor libraries do
// (rocsparse_spmm_stage_preprocess). A plan looks at the matrix ONCE and keeps what every later launch can reuse:
//
//   * the longest row (decides the long-row pass exactly instead of guessing from nnz and the mean degree);
//   * for dense graphs: the workspace with the per-row split points of the cache-blocked path;
//   * for sparse graphs whose B exceeds the L2s: a ROW-CLUSTERED copy of the matrix (reorder.cpp) and a task
//     table with an equal non-zero budget per wavefront. Rows that share neighbours are processed next to
//     each other, so the B rows they share are gathered from the XCD's L2 instead of crossing the fabric
//     again. Only the processing order changes: every row is still summed by one lane group in its own CSR
//     order and written to its own C row (through perm[]), so the result has the same bits as the plain call;
//   * tables of the staged-rows, column-slab and padded-record kernels for the plan's width, where the policy keeps them.
//
// How the file is laid out:
//   * WHICH KERNEL a launch takes is one pure function, plan_route (plan_policy.cpp). plan_run switches on its answer,
//     gespmm_plan_describe prints it, gespmm_plan_tune asks it which candidates exist: they cannot disagree.
//   * OWNERSHIP: every device allocation has one owning member of gespmm_plan, released by its destructor; pointers into an
//     allocation are views. Creation holds the plan in a unique_ptr, so every early exit is a plain return.
//   * CREATION is a sequence of stages (plan_create_impl): facts -> order (device or host analysis) -> task tables and
//     values -> staged / slab tables -> launch scratch -> record tables.
//
// The plan refers to the caller's arrays only while it is created (and in gespmm_plan_set_values) — unless it keeps the
// storage order, in which case it launches on them.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../../include/gespmm.h"
#include "auto_plan.h"
#include "plan.h"
#include "plan_device.h"
#include "plan_policy.h"
#include "reorder.h"
#include "sddmm_heads.h"
#include "select.h"
#include "spmm_device.h"
#include "spmm_heads.h"
#include "spmm_kernels.h"

struct gespmm_plan {
    int64_t M = 0, K = 0, nnz = 0, N = 0;
    int variant = GESPMM_VARIANT_AUTO;
    int launch_flags = 0;
    int device = 0;
    const int32_t* rowptr = nullptr;  // caller's arrays (used only when the plan keeps the storage order)
    const int32_t* colind = nullptr;
    const float* val = nullptr;
    bool valued = false;
    int32_t max_degree = 0;
    bool reordered = false;
    bool identity_order = false;  // reordered, but the plan's copy is in the caller's order (a matrix that arrived clustered: the staged-rows kernel needs the plan's tables)
    // ---- device memory: OWNERS (released by the destructor) and views into them (never freed)
    void* d_block = nullptr;          // owner: the plan's permuted copy — perm / rowptr / colind / src_begin (/ val) are parts of this ONE allocation
    int32_t* d_rowptr = nullptr;      // views (alloc_plan_copy)
    int32_t* d_colind = nullptr;
    int32_t* d_perm = nullptr;
    int32_t* d_src_begin = nullptr;
    float* d_val = nullptr;           // view: into d_block when the plan was created with values, else d_val_late
    float* d_val_late = nullptr;      // owner: gespmm_plan_set_values gave values to a plan created without (the block has no room for them)
    int32_t* d_tasks = nullptr;       // owner: the block of both task tables
    int32_t ntasks = 0;
    int32_t* d_gtasks = nullptr;      // view: lane-group tasks of the segmented-stream kernel
    int32_t ngtasks = 0;
    void* ws = nullptr;               // owner: scratch of the launches
    int64_t ws_bytes = 0;
    // owners, SDDMM through the plan (built on first use): edges in clustered order as COO with the ORIGINAL row ids, the
    // position of every edge in the caller's CSR, and a buffer for the results in clustered order
    int32_t* d_coo_row = nullptr;
    int32_t* d_coo_row_storage = nullptr;  // storage-order plans: row id of every edge (the COO form skips the row search)
    int32_t* d_edge_dst = nullptr;
    float* d_sddmm_tmp = nullptr;
    int32_t task_entries = 0;
    int kernel_choice = 0;         // GESPMM_PLAN_KERNEL_*
    gespmm::PlanFacts facts;       // what the policy functions (plan_policy.h) are asked with
    std::vector<int32_t> perm_host;  // filled by the host analysis, or on demand (gespmm_plan_get_order)
    bool cost_skipped = false;       // AUTO skipped the analysis: expected launches x estimated gain < estimated cost (plan_policy.cpp)
    double est_gain_us = 0.0, est_cost_us = 0.0;
    int analysis = 0;                // GESPMM_PLAN_ANALYSIS_*
    double model_seconds = 0.0;
    bool split_ready = false;
    int split_vec = 0;               // vector width (operand alignment) the kept split points were computed for
    gespmm::ClusterStats stats;
    double analysis_seconds = 0.0, cluster_seconds = 0.0;
    double hits_before = -1.0, hits_after = -1.0;
    // staged-rows kernel (spmm_staged.hip): tables for width N (plan_device.hip: device_build_staging)
    gespmm::StagingTables stg;
    double staging_seconds = 0.0;
    // column-slab tables (round 6; dense clustered matrices at N = 128): staged tables of the slab view, one launch per slab (plan_run)
    gespmm::StagingTables slab;
    gespmm::SlabView slab_view;
    double slab_seconds = 0.0;
    // padded-record kernel (spmm_records.hip): tables for width N (narrow widths, short rows)
    gespmm::RecordTables rec;
    double records_seconds = 0.0;
    // gespmm_plan_tune: measured kernel times on the caller's operands (us; < 0: candidate not available)
    // The measurement is valid for the plan's own width only: launches at p->N take tuned_kernel / tuned_vec, every other width keeps
    // the per-launch rules of plan_policy.cpp (kernel_choice stays what the creator asked for).
    bool tuned = false;
    int tuned_kernel = 0;  // GESPMM_PLAN_KERNEL_* that won (valid while `tuned`)
    int tuned_vec = 0;     // 1: the winner is the batch-stream kernel with 4 floats per lane (N <= 64)
    bool staging_kept_by_policy = false;  // keep_staged_tables() said yes at creation (else the tables exist only while tune measures them / if they won)
    double tune_us[5] = {-1.0, -1.0, -1.0, -1.0, -1.0};  // batch-stream, segmented-stream, staged-rows, batch-stream with 4 floats per lane (N <= 64), padded records
    // the fused product's composition route (gespmm_plan_spmm_fused_f32): K x N floats for col_scale . B, made by the first call that needs them
    float* d_fused_scratch = nullptr;  // owner
    int64_t fused_scratch_bytes = 0;
    // 16-bit operands, composition route (gespmm_plan_spmm_x16): K x N floats for widen(B), M x N for the fp32 product; made by the first call
    // that needs them (and again by a wider one)
    float* d_x16_b = nullptr;  // owners
    float* d_x16_c = nullptr;
    int64_t x16_b_bytes = 0, x16_c_bytes = 0;
    int x16_last_route = -1;   // what the last 16-bit call RAN (-1: none yet), its width, element type and lane geometry: gespmm_plan_describe
    gespmm::Geometry x16_last_geo = {};
    int64_t x16_last_N = 0;
    int x16_last_dtype = 0;
    // the multi-head product (gespmm_plan_spmm_heads_f32): the caller's [nnz, H] weights in the plan's entry order, rewritten by every call;
    // made by the first call on a clustered plan and again when H grows
    float* d_heads_val = nullptr;  // owner
    int64_t heads_val_bytes = 0;
    // the multi-head SDDMM on the clustered edge order (gespmm_plan_sddmm_heads_f32, route 2): [nnz, H] results before the scatter; made
    // by the first such call and again when H grows, never on a capturing stream
    float* d_sddmm_heads_tmp = nullptr;  // owner
    int64_t sddmm_heads_tmp_bytes = 0;
    int heads_last_route = -1;  // what the last multi-head call RAN (-1: none yet), its H and F and the kernel's lane geometry: gespmm_plan_describe
    gespmm::Geometry heads_last_geo = {};
    int64_t heads_last_H = 0, heads_last_F = 0;
    bool records_kept_by_policy = false;  // want_record_tables() / keep_record_tables() said yes at creation (else the tables exist only while tune measures them / if they won)

    gespmm_plan() = default;
    gespmm_plan(const gespmm_plan&) = delete;
    gespmm_plan& operator=(const gespmm_plan&) = delete;
    ~gespmm_plan() {
        gespmm::free_staging(&stg);
        gespmm::free_staging(&slab);
        gespmm::free_slab_view(&slab_view, false);
        gespmm::free_records(&rec);
        for (void* q : {d_block, (void*)d_val_late, (void*)d_tasks, ws, (void*)d_coo_row, (void*)d_coo_row_storage, (void*)d_edge_dst, (void*)d_sddmm_tmp, (void*)d_fused_scratch, (void*)d_x16_b, (void*)d_x16_c, (void*)d_heads_val, (void*)d_sddmm_heads_tmp})
            if (q) (void)hipFree(q);
    }
};

namespace {

__global__ void permute_values_kernel(const int32_t* __restrict__ rowptr_p, const int32_t* __restrict__ src_begin,
                                      const float* __restrict__ val, float* __restrict__ val_p, int M, int nnz) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const int r = gespmm::row_of_entry(rowptr_p, M, p);
    val_p[p] = val[src_begin[r] + (p - rowptr_p[r])];
}

__global__ void plan_edge_maps_kernel(const int32_t* __restrict__ rowptr_p, const int32_t* __restrict__ src_begin,
                                      const int32_t* __restrict__ perm, int32_t* __restrict__ coo_row,
                                      int32_t* __restrict__ edge_dst, int M, int nnz) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const int r = gespmm::row_of_entry(rowptr_p, M, p);
    coo_row[p] = perm[r];
    edge_dst[p] = src_begin[r] + (p - rowptr_p[r]);
}

__global__ void expand_rows_kernel(const int32_t* __restrict__ rowptr, int32_t* __restrict__ coo_row, int M, int nnz) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < nnz) coo_row[p] = gespmm::row_of_entry(rowptr, M, p);
}

__global__ void scatter_by_index_kernel(const float* __restrict__ src, const int32_t* __restrict__ dst_index,
                                        float* __restrict__ dst, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[dst_index[i]] = src[i];
}

inline bool aligned16(const float* B, const float* C) {  // what the staged-rows and padded-record kernels ask of their operands
    return ((reinterpret_cast<uintptr_t>(B) | reinterpret_cast<uintptr_t>(C)) & 15) == 0;
}

struct Stopwatch {
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double seconds() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};

// The plan's permuted copy of the matrix as ONE allocation (a hipMalloc costs ~0.1 ms: five of them were 7 % of the device analysis).
hipError_t alloc_plan_copy(gespmm_plan* p) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t entries = (size_t)(p->nnz > 0 ? p->nnz : 1);
    const size_t b_perm = up((size_t)p->M * 4), b_rp = up(((size_t)p->M + 1) * 4), b_ci = up(entries * 4), b_src = up((size_t)p->M * 4),
                 b_val = p->valued ? up(entries * 4) : 0;
    const hipError_t e = hipMalloc(&p->d_block, b_perm + b_rp + b_ci + b_src + b_val);
    if (e != hipSuccess) return e;
    char* base = reinterpret_cast<char*>(p->d_block);
    p->d_perm = reinterpret_cast<int32_t*>(base);
    p->d_rowptr = reinterpret_cast<int32_t*>(base + b_perm);
    p->d_colind = reinterpret_cast<int32_t*>(base + b_perm + b_rp);
    p->d_src_begin = reinterpret_cast<int32_t*>(base + b_perm + b_rp + b_ci);
    if (p->valued) p->d_val = reinterpret_cast<float*>(base + b_perm + b_rp + b_ci + b_src);
    return hipSuccess;
}

// ... and gone again, with the task tables cut from it: the plan launches on the caller's arrays (nothing is paid per launch)
void drop_plan_copy(gespmm_plan* p) {
    if (p->d_block) (void)hipFree(p->d_block);
    if (p->d_tasks) (void)hipFree(p->d_tasks);
    p->d_block = nullptr;
    p->d_perm = p->d_rowptr = p->d_colind = p->d_src_begin = p->d_tasks = p->d_gtasks = nullptr;
    p->d_val = nullptr;
    p->ntasks = p->ngtasks = 0;
}

hipError_t permute_values(const gespmm_plan* p, const float* val, hipStream_t st) {  // d_val = val in the plan's entry order
    hipLaunchKernelGGL(permute_values_kernel, dim3((unsigned)((p->nnz + 255) / 256)), dim3(256), 0, st, p->d_rowptr, p->d_src_begin, val,
                       p->d_val, (int)p->M, (int)p->nnz);
    return hipGetLastError();
}

// Experiment knobs (scripts/plan_time.py): GESPMM_CLUSTER_LEVELS / _SWEEPS / _STOP / _CAP override the clustering defaults.
gespmm::ClusterOptions cluster_options_from_env() {
    gespmm::ClusterOptions o;
    if (const char* v = getenv("GESPMM_CLUSTER_LEVELS")) o.max_levels = atoi(v);
    if (const char* v = getenv("GESPMM_CLUSTER_SWEEPS")) o.sweeps = atoi(v);
    if (const char* v = getenv("GESPMM_CLUSTER_STOP")) o.stop_percent = atoi(v);
    if (const char* v = getenv("GESPMM_CLUSTER_CAP")) o.first_cap = atoi(v);
    return o;
}

// ... for a plan: what the environment leaves open, the policy fills in
gespmm::ClusterOptions cluster_options_for(const gespmm::PlanFacts& f, int threads) {
    gespmm::ClusterOptions o = cluster_options_from_env();
    if (o.max_levels <= 0) o.max_levels = gespmm::cluster_levels_for(f);
    if (o.sweeps <= 0) o.sweeps = gespmm::cluster_sweeps_for(f);
    o.threads = threads;
    return o;
}

// GESPMM_PLAN_TIMING: the time since the previous lap of this thread, device work included (what == NULL: start)
void lap(hipStream_t st, const char* what) {
    static const bool timing = getenv("GESPMM_PLAN_TIMING") != nullptr;
    if (!timing) return;
    (void)hipStreamSynchronize(st);
    static thread_local std::chrono::steady_clock::time_point last;
    const auto now = std::chrono::steady_clock::now();
    if (what) fprintf(stderr, "[plan] %-22s %8.3f ms\n", what, std::chrono::duration<double>(now - last).count() * 1e3);
    last = now;
}

// What a launch of width N does (plan_policy.cpp: plan_route) — the plan's state as that function reads it.
gespmm::RouteAnswer route_of(const gespmm_plan* p, int64_t N, int reduce, bool operands_aligned16) {
    gespmm::RouteState s;
    s.reordered = p->reordered;
    s.has_staged = p->stg.ev != nullptr;
    s.has_slabs = p->slab.ev != nullptr;
    s.has_records = p->rec.batches != nullptr;
    s.has_gtasks = p->d_gtasks != nullptr;
    s.staging_kept_by_policy = p->staging_kept_by_policy;
    s.tuned = p->tuned;
    s.tuned_kernel = p->tuned_kernel;
    s.tuned_vec = p->tuned_vec;
    s.kernel_choice = p->kernel_choice;
    s.hits_after = p->hits_after;
    s.stg_waves = p->stg.waves;
    s.stg_slots = p->stg.slots;
    s.stg_nlong = p->stg.nlong;
    return gespmm::plan_route(p->facts, s, N, reduce, operands_aligned16);
}

// The matrix a streaming launch of the plan works on, for the route's answer: a clustered plan's copy with both task tables (which
// streaming kernel: ra.segmented; which lane geometry at narrow widths: ra.vec4 — plan_policy.cpp), else the caller's arrays.
gespmm::CsrView plan_view(const gespmm_plan* p, const gespmm::RouteAnswer& ra) {
    if (!p->reordered) return gespmm::csr_view(p->rowptr, p->colind, p->valued ? p->val : nullptr, p->M, p->K, p->nnz, p->variant);
    gespmm::CsrView A = gespmm::csr_view(p->d_rowptr, p->d_colind, p->valued ? p->d_val : nullptr, p->M, p->K, p->nnz,
                                         ra.vec4 ? GESPMM_VARIANT_CRC_CWM4 : p->variant);
    A.planned = true;
    A.pl = {p->d_tasks, p->ntasks, p->d_perm, p->d_gtasks, p->ngtasks, ra.segmented};
    return A;
}

// A buffer the plan owns (one of the destructor's list), made at least `need` bytes by the call that needs it. resize_owned: the old
// block goes first — hipFree synchronises, no earlier launch still uses it — and what the plan holds stays consistent when hipMalloc
// fails. grow_owned: the same, never on a capturing stream (hipErrorStreamCaptureUnsupported: nothing touched, the caller launches nothing).
hipError_t resize_owned(float** q, int64_t* have, int64_t need) {
    if (*have >= need) return hipSuccess;
    if (*q) (void)hipFree(*q);
    *q = nullptr;
    *have = 0;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(q), (size_t)need);
    if (e == hipSuccess) *have = need;
    return e;
}
int grow_owned(float** q, int64_t* have, int64_t need, hipStream_t st) {
    if (*have >= need) return 0;
    const int rc = gespmm::refuse_allocation_under_capture(st);
    return rc != 0 ? rc : (int)resize_owned(q, have, need);
}

}  // namespace

namespace gespmm {
bool plan_is_clustered(const gespmm_plan* p) { return p && p->reordered; }
static std::atomic<bool> g_analysis_warm{false};
bool analysis_is_warm() { return g_analysis_warm.load(std::memory_order_relaxed); }
void mark_analysis_warm() { g_analysis_warm.store(true, std::memory_order_relaxed); }
}  // namespace gespmm

extern "C" {

int gespmm_cluster_rows(const int32_t* rowptr, const int32_t* colind, int64_t M, int64_t K, int32_t threads,
                        int32_t* perm_out, int32_t* levels_out, int32_t* clusters_out /* [16] */) {
    if (M < 0 || K < 0 || (M > 0 && (!rowptr || !perm_out))) return GESPMM_EINVAL;
    gespmm::ClusterOptions opt;
    opt.threads = threads;
    gespmm::ClusterStats st;
    try {
        if (gespmm::cluster_rows(M, K, rowptr, colind, opt, perm_out, &st) != 0) return GESPMM_EINVAL;
    } catch (const std::bad_alloc&) {
        return GESPMM_ENOMEM;
    }
    if (levels_out) *levels_out = st.levels;
    if (clusters_out)
        for (int i = 0; i < 16; ++i) clusters_out[i] = st.clusters[i];
    return 0;
}

// Study hook (scripts/cluster_chain_study.py): the host clustering with its options and the coarsest cluster of every row.
int gespmm_cluster_rows_study(const int32_t* rowptr, const int32_t* colind, int64_t M, int64_t K, int32_t max_levels, int32_t sweeps,
                              int32_t* perm_out, int32_t* top_label_out, int32_t* clusters_out /* [16] */) {
    if (M <= 0 || !rowptr || !perm_out) return GESPMM_EINVAL;
    gespmm::ClusterOptions opt = cluster_options_from_env();
    opt.max_levels = max_levels;
    opt.sweeps = sweeps;
    gespmm::ClusterStats st;
    if (gespmm::cluster_rows(M, K, rowptr, colind, opt, perm_out, &st, top_label_out) != 0) return GESPMM_EINVAL;
    if (clusters_out)
        for (int i = 0; i < 16; ++i) clusters_out[i] = st.clusters[i];
    return st.levels;
}

double gespmm_simulate_l2_hits(const int32_t* rowptr, const int32_t* colind, int64_t M, int64_t K, const int32_t* perm,
                               int32_t slices, int64_t window_rows) {
    if (M <= 0 || K <= 0 || !rowptr || slices < 1 || window_rows < 1) return 0.0;
    try {
        return gespmm::simulate_l2_hits(M, K, rowptr, colind, perm, slices, window_rows);
    } catch (const std::bad_alloc&) {
        return -1.0;
    }
}

// The device analysis by itself (DEVICE rowptr / colind, HOST outputs) — what tests compare with gespmm_cluster_rows.
int gespmm_device_cluster_rows(const int32_t* rowptr, const int32_t* colind, int64_t M, int64_t K, int64_t nnz,
                               int32_t* perm_out_host, int32_t* levels_out, int32_t* clusters_out /* [16] */, void* stream) {
    if (M < 0 || K < 0 || nnz < 0 || (M > 0 && (!rowptr || !perm_out_host)) || (nnz > 0 && !colind)) return GESPMM_EINVAL;
    if (M == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int32_t max_deg = 0, bad = 0;
    hipError_t e = gespmm::device_validate_csr(rowptr, colind, M, K, nnz, &max_deg, &bad, nullptr, st);
    if (e != hipSuccess) return (int)e;
    if (bad) return GESPMM_EINVAL;
    int32_t* d_perm = nullptr;
    e = hipMalloc(reinterpret_cast<void**>(&d_perm), (size_t)M * 4);
    if (e != hipSuccess) return (int)e;
    gespmm::ClusterOptions opt;
    gespmm::ClusterStats stats;
    e = gespmm::device_cluster_rows(M, K, nnz, rowptr, colind, opt, d_perm, &stats, st);
    if (e == hipSuccess) e = hipMemcpyAsync(perm_out_host, d_perm, (size_t)M * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(d_perm);
    if (e != hipSuccess) return (int)e;
    if (levels_out) *levels_out = stats.levels;
    if (clusters_out)
        for (int i = 0; i < 16; ++i) clusters_out[i] = stats.clusters[i];
    return 0;
}

// The device L2 model by itself: DEVICE rowptr / colind, perm_host (HOST, may be NULL = storage order). Returns the
// modelled hit rate, or a negative value on error.
double gespmm_device_l2_model(const int32_t* rowptr, const int32_t* colind, int64_t M, int64_t K, int64_t nnz,
                              const int32_t* perm_host, int32_t slices, int64_t window_rows, int64_t max_entries_per_slice,
                              int32_t samples_per_slice, void* stream) {
    if (M <= 0 || K <= 0 || nnz <= 0 || !rowptr || !colind || slices < 1 || slices > 16 || window_rows < 1) return -1.0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double hits = -1.0;
    hipError_t e = hipSuccess;
    int32_t *d_perm = nullptr, *rp = nullptr, *ci = nullptr, *src = nullptr;
    if (perm_host) {
        e = hipMalloc(reinterpret_cast<void**>(&d_perm), (size_t)M * 4);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&rp), ((size_t)M + 1) * 4);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&ci), (size_t)nnz * 4);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&src), (size_t)M * 4);
        if (e == hipSuccess) e = hipMemcpyAsync(d_perm, perm_host, (size_t)M * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = gespmm::device_permute_csr(M, nnz, rowptr, colind, d_perm, rp, ci, src, st);
    }
    if (e == hipSuccess)
        e = gespmm::device_l2_model(M, K, nnz, perm_host ? rp : rowptr, perm_host ? ci : colind, slices, window_rows,
                                    max_entries_per_slice, samples_per_slice > 0 ? samples_per_slice : 8192, &hits, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    for (void* q : {(void*)d_perm, (void*)rp, (void*)ci, (void*)src})
        if (q) (void)hipFree(q);
    return e == hipSuccess ? hits : -1.0;
}

// Test hook: the task table of a clustered plan (which = 0: wavefront tasks, 1: lane-group tasks) as int4 records in
// HOST memory; returns the number of tasks (<= capacity are copied) or a negative error.
int gespmm_plan_debug_tasks(const gespmm_plan* p, int32_t which, int32_t* out_host, int64_t capacity) {
    if (!p || which < 0 || which > 1) return GESPMM_EINVAL;
    if (!p->reordered) return 0;
    const int32_t n = which ? p->ngtasks : p->ntasks;
    const int32_t* d = which ? p->d_gtasks : p->d_tasks;
    const int64_t take = n < capacity ? n : capacity;
    if (take > 0 && out_host && hipMemcpy(out_host, d, (size_t)take * 16, hipMemcpyDeviceToHost) != hipSuccess) return GESPMM_EINVAL;
    return n;
}

// Test hook: the staging lists of the plan's staged-rows tables (blocks x slots columns, -1 = unused) in HOST memory.
int64_t gespmm_plan_debug_staging(const gespmm_plan* p, int32_t* info_host, int32_t* out_host, int64_t capacity) {
    if (!p) return GESPMM_EINVAL;
    if (!p->stg.ev || !p->stg.hot_cols) return 0;
    const int64_t n = (int64_t)p->stg.nblocks * p->stg.slots;
    if (info_host) {
        info_host[0] = p->stg.nblocks;
        info_host[1] = p->stg.slots;
        info_host[2] = p->stg.rows;
        info_host[3] = p->stg.fill_window;
    }
    const int64_t take = n < capacity ? n : capacity;
    if (take > 0 && out_host && hipMemcpy(out_host, p->stg.hot_cols, (size_t)take * 4, hipMemcpyDeviceToHost) != hipSuccess) return GESPMM_EINVAL;
    return n;
}

// Tables of the staged-rows kernel for the plan's width (plan_device.hip). Hub rows (one wavefront would walk such a row
// alone) are taken out: the staged kernel sees them empty, the streaming kernel's long-row pass gets them as one-row tasks
// (plan_run). Leaves p->stg empty when there is nothing but hub rows.
static hipError_t build_staging_tables(gespmm_plan* p, hipStream_t st) {
    const Stopwatch sw;
    const int64_t M = p->M, K = p->K, nnz = p->nnz, N = p->N;
    gespmm::StagedShape shape = gespmm::staged_block_shape(N);  // (the block shape of whichever staged kernel serves the width)
    shape.rows = gespmm::staged_rows_for(p->facts, shape);     // (by mean degree: plan_policy.cpp)
    hipError_t e = hipSuccess;
    const int32_t* rp_s = p->d_rowptr;
    const int32_t* ci_s = p->d_colind;
    const float* val_s = p->valued ? p->d_val : nullptr;
    int32_t* ci_tmp = nullptr;
    float* val_tmp = nullptr;
    int64_t nnz_s = nnz;
    if (p->max_degree > gespmm::kStagedMaxRow) {
        e = gespmm::device_split_long_rows(M, nnz, p->d_rowptr, p->d_colind, val_s, gespmm::kStagedMaxRow, &p->stg, &ci_tmp, &val_tmp, st);
        rp_s = p->stg.rowptr_s;
        ci_s = ci_tmp;
        val_s = val_tmp;
        nnz_s = p->stg.nnz_s;
    }
    // the fill pass's window (plan_policy.cpp: staged_fill_window) — GESPMM_STAGED_FILL overrides it, read per plan so that one process
    // can build the same plan with and without the pass (0: none)
    int fill = gespmm::staged_fill_window(p->facts, shape);
    if (const char* fe = getenv("GESPMM_STAGED_FILL")) fill = M == K ? atoi(fe) : 0;
    fill = fill < 0 ? 0 : (fill > gespmm::kStagedFillMaxWindow ? gespmm::kStagedFillMaxWindow : fill);
    if (e == hipSuccess && nnz_s > 0)
        e = gespmm::device_build_staging(M, K, nnz_s, rp_s, ci_s, val_s, p->d_perm, shape.rows, shape.slots, shape.waves,
                                         shape.tasks_per_block, &p->stg, st, 0, false, fill);
    if (ci_tmp) (void)hipFree(ci_tmp);
    if (val_tmp) (void)hipFree(val_tmp);
    if (e == hipSuccess && !p->stg.ev) gespmm::free_staging(&p->stg);  // (nothing but hub rows)
    p->staging_seconds = sw.seconds();
    return e;
}

// Column-slab tables (plan_device.hip: device_build_slab_view): the clustered matrix as P ascending column ranges, staged tables per
// (block of rows, slab). Leaves p->slab empty when the matrix does not qualify (a row with descending columns: slab order would not be
// CSR order; a slab of some row beyond the staged kernel's row limit) — the plan's other kernels stay.
static hipError_t build_slab_tables(gespmm_plan* p, int P, hipStream_t st) {
    const Stopwatch sw;
    const int64_t M = p->M, K = p->K, nnz = p->nnz, N = p->N;
    gespmm::StagedShape shape = gespmm::staged_block_shape(N);
    static const int rows_env = getenv("GESPMM_SLAB_ROWS") ? atoi(getenv("GESPMM_SLAB_ROWS")) : 0;  // experiments
    if (rows_env > 0) shape.rows = rows_env;
    if (N != 128 || shape.waves != 16 || shape.slots != 160 || P < 2 || nnz <= 0 || !gespmm::staged_serves(M, K, N) ||
        !gespmm::staged_stream_fits(M * P, nnz) || M * P >= (1ll << 30))
        return hipSuccess;
    hipError_t e = gespmm::device_build_slab_view(M, K, nnz, p->d_rowptr, p->d_colind, p->valued ? p->d_val : nullptr, p->d_perm, P,
                                                  &p->slab_view, st);
    if (e == hipSuccess && (!p->slab_view.sorted || p->slab_view.max_row > gespmm::kStagedMaxRow)) {
        gespmm::free_slab_view(&p->slab_view, false);
        return hipSuccess;
    }
    if (e == hipSuccess)
        e = gespmm::device_build_staging(M * P, K, nnz, p->slab_view.rowptr_v, p->slab_view.colind_v, p->slab_view.val_v, p->slab_view.perm_v,
                                         shape.rows, shape.slots, shape.waves, shape.waves, &p->slab, st, M, true);
    gespmm::free_slab_view(&p->slab_view, e == hipSuccess);  // (the view's column indices / values / row map are in the tables now)
    if (e != hipSuccess) gespmm::free_staging(&p->slab);
    p->slab_seconds = sw.seconds();
    return e;
}

static double record_slot_fill(const gespmm_plan* p) {  // share of the entry slots of the batches that carry an entry
    if (!p->rec.batches || p->rec.nbatches <= 0) return 0.0;
    return (double)p->nnz / ((double)p->rec.nbatches * (64 / p->rec.group) * gespmm::kRecordPiece);
}

// Tables of the padded-record kernel (spmm_records.hip) for the plan's width: the matrix in the order the plan processes it (its
// clustered copy, or the caller's arrays when the storage order was kept).
static hipError_t build_record_tables(gespmm_plan* p, hipStream_t st) {
    const Stopwatch sw;
    static const int env_rows = getenv("GESPMM_REC_BATCHES") ? atoi(getenv("GESPMM_REC_BATCHES")) : 0;  // experiments
    const int rows = env_rows > 0 ? env_rows : gespmm::records_batches_per_task(p->facts);
    const hipError_t e = gespmm::device_build_records(p->M, p->reordered ? p->d_rowptr : p->rowptr, p->reordered ? p->d_colind : p->colind,
                                                      p->valued ? (p->reordered ? p->d_val : p->val) : nullptr,
                                                      p->reordered ? p->d_perm : nullptr, rows, p->N, &p->rec, st);
    p->records_seconds = sw.seconds();
    return e;
}

// ------------------------------------------------------------------------------------------------ creation, stage by stage
// Every stage returns 0 or an error code (GESPMM_E* or a hipError_t); what the plan owns by then goes with the plan.

struct Creation {  // what the stages hand on
    hipStream_t st = nullptr;
    bool on_host = false;
    int threads = 0;                           // gespmm_plan_options.threads (host clustering)
    gespmm::AnalysisDecision ad;
    std::vector<int32_t> h_rowptr, h_colind;   // host analysis: the caller's matrix
    std::vector<int32_t> rp, ci, src;          // host analysis: its row-permuted copy ...
    std::vector<int32_t> tasks, gtasks;        // ... and task tables, alive until the uploads are synchronised (make_task_tables)
};

static int check_create_args(const int32_t* rowptr, const int32_t* colind, int64_t M, int64_t K, int64_t nnz, int64_t N, int variant,
                             const gespmm_plan_options* opt) {
    const int rc = gespmm::check_csr_sizes(M, K, N, nnz, 0);
    if (rc != 0) return rc;
    if (!gespmm::valid_variant(variant)) return GESPMM_EINVAL;
    if (M > 0 && !rowptr) return GESPMM_EINVAL;
    if (nnz > 0 && !colind) return GESPMM_EINVAL;
    if (!opt) return 0;
    if (opt->reorder < 0 || opt->reorder > 2) return GESPMM_EINVAL;
    const int k = opt->kernel;
    if (k != GESPMM_PLAN_KERNEL_AUTO && k != GESPMM_PLAN_KERNEL_STREAM && k != GESPMM_PLAN_KERNEL_SEG_STREAM && k != GESPMM_PLAN_KERNEL_STAGED &&
        k != GESPMM_PLAN_KERNEL_RECORDS && k != GESPMM_PLAN_KERNEL_STAGED_SLABS)
        return GESPMM_EINVAL;
    if (opt->expected_launches < 0) return GESPMM_EINVAL;
    if (opt->analysis != GESPMM_PLAN_ANALYSIS_DEVICE && opt->analysis != GESPMM_PLAN_ANALYSIS_HOST) return GESPMM_EINVAL;
    return 0;
}

// One pass over the matrix on the device — rowptr monotone and consistent with nnz, every column index inside [0, K) (the kernels
// trust them), the longest row — then the facts the policy is asked with (plan_policy.h) and its decision about the analysis.
static int validate_and_decide(gespmm_plan* p, Creation& cx, const gespmm_plan_options* opt) {
    const int64_t M = p->M, K = p->K, nnz = p->nnz, N = p->N;
    const int reorder_mode = opt ? opt->reorder : GESPMM_PLAN_REORDER_AUTO;
    int32_t max_deg = 0, bad = 0;
    double wedge_probe = -1.0;
    hipError_t e = gespmm::device_validate_csr(p->rowptr, p->colind, M, K, nnz, &max_deg, &bad,
                                               (reorder_mode == GESPMM_PLAN_REORDER_AUTO && !cx.on_host) ? &wedge_probe : nullptr, cx.st);
    if (e != hipSuccess) return (int)e;
    if (bad) return GESPMM_EINVAL;  // rowptr does not describe nnz entries, or a column index is outside [0, K)
    if (cx.on_host) {  // the matrix comes to the host once
        cx.h_rowptr.assign((size_t)M + 1, 0);
        cx.h_colind.resize((size_t)nnz);
        if (M > 0) e = hipMemcpyAsync(cx.h_rowptr.data(), p->rowptr, ((size_t)M + 1) * 4, hipMemcpyDeviceToHost, cx.st);
        if (e == hipSuccess && nnz > 0) e = hipMemcpyAsync(cx.h_colind.data(), p->colind, (size_t)nnz * 4, hipMemcpyDeviceToHost, cx.st);
        if (e == hipSuccess) e = hipStreamSynchronize(cx.st);
        if (e != hipSuccess) return (int)e;
    }
    p->max_degree = max_deg;
    // what a plain call would launch, the longest row, the options
    gespmm::PlanFacts& f = p->facts;
    f.M = M;
    f.K = K;
    f.nnz = nnz;
    f.N = N;
    f.variant = p->variant;
    f.max_degree = max_deg;
    f.reorder_mode = reorder_mode;
    f.kernel_choice = p->kernel_choice = opt ? opt->kernel : GESPMM_PLAN_KERNEL_AUTO;
    f.host_analysis = cx.on_host;
    f.user_flags = opt ? opt->flags : 0;
    f.opt_task_entries = opt ? opt->task_entries : 0;
    f.opt_row_floor = opt ? opt->row_floor : 0;
    f.expected_launches = opt ? opt->expected_launches : 0;
    f.wedge_probe = wedge_probe;
    f.cold_start = !gespmm::analysis_is_warm();
    gespmm::Selection sel;
    const int max_vec = gespmm::vec_limit(N, 16);
    const int lr_flags = gespmm::long_row_flags(M, nnz, max_deg, f.user_flags);
    if (gespmm::resolve_geometry(M, K, N > 0 ? N : 1, nnz, p->variant, max_vec, 0, 0, 0, 0, 0, lr_flags, &sel) != 0) return GESPMM_EINVAL;
    f.sel_variant = sel.variant;
    f.slab_blocked = sel.geo.slab_blocked;
    f.tile_cols = (int64_t)sel.geo.group * sel.geo.vec * sel.geo.strips;
    cx.ad = gespmm::decide_analysis(f);
    p->launch_flags = cx.ad.launch_flags;
    p->cost_skipped = cx.ad.cost_skipped;
    p->est_gain_us = cx.ad.cost.gain_us;
    p->est_cost_us = cx.ad.cost.cost_us;
    return 0;
}

// Analysis on the device: cluster, copy the matrix in the new order, model the L2s on both orders. *clustered: the plan holds a
// permuted copy (in the clustered order — or in the caller's, identity_order) and goes on to its task tables; else it holds nothing.
static int order_on_device(gespmm_plan* p, const Creation& cx, bool* clustered) {
    const int64_t M = p->M, K = p->K, nnz = p->nnz;
    const gespmm::PlanFacts& f = p->facts;
    hipStream_t st = cx.st;
    lap(st, nullptr);
    const Stopwatch tc;
    hipError_t e = alloc_plan_copy(p);
    const gespmm::ClusterOptions copt = cluster_options_for(f, 0);
    if (e == hipSuccess) e = gespmm::device_cluster_rows(M, K, nnz, p->rowptr, p->colind, copt, p->d_perm, &p->stats, st);
    p->cluster_seconds = tc.seconds();
    lap(st, "cluster");
    if (e == hipSuccess) e = gespmm::device_permute_csr(M, nnz, p->rowptr, p->colind, p->d_perm, p->d_rowptr, p->d_colind, p->d_src_begin, st);
    lap(st, "permute");
    const Stopwatch tm;
    // (the storage order is only judged against the clustered one — "already local, or hit by hubs: keep it" shows anywhere in a
    //  slice — so on matrices of >= 2^20 entries the first QUARTER of every slice is modelled: a quarter of the sort)
    const int64_t model_sample = cx.ad.model_sample;
    const int64_t before_sample = nnz >= (1 << 20) ? std::max<int64_t>(nnz / 32, 1 << 15) : model_sample;
    const int model_points = gespmm::model_points_for(f);  // sampled accesses per slice
    if (e == hipSuccess)
        e = gespmm::device_l2_model(M, K, nnz, p->rowptr, p->colind, 8, cx.ad.model_window,
                                    model_sample > 0 ? std::min<int64_t>(model_sample, before_sample) : before_sample, model_points,
                                    &p->hits_before, st);
    if (e == hipSuccess)
        e = gespmm::device_l2_model(M, K, nnz, p->d_rowptr, p->d_colind, 8, cx.ad.model_window, model_sample, model_points, &p->hits_after, st);
    p->model_seconds = tm.seconds();
    lap(st, "l2 model x2");
    if (e != hipSuccess) return (int)e;
    if (gespmm::keep_clustered_order(f, cx.ad, p->hits_before, p->hits_after)) {
        if (cx.ad.dense_try) p->launch_flags |= GESPMM_FLAG_NO_SLAB_BLOCKED;  // a clustered dense graph runs the streaming kernels
    } else if (!cx.ad.dense_try && gespmm::storage_order_wants_plan_copy(f, p->hits_before)) {
        // The matrix ARRIVED in an order as good as the clustering's (a caller who keeps the graph by community): the staged-rows
        // kernel still needs the plan's own tables, so the plan copies the matrix in the IDENTITY order and goes on as if it had
        // clustered it (dropped again in build_device_tables if the tables are not kept: then nothing is paid per launch, as before)
        e = gespmm::device_identity_copy(M, nnz, p->rowptr, p->colind, p->d_perm, p->d_rowptr, p->d_colind, p->d_src_begin, st);
        if (e != hipSuccess) return (int)e;
        p->hits_after = p->hits_before;
        p->identity_order = true;
    } else {
        drop_plan_copy(p);  // the storage order (or the cache-blocked path) is as good: keep it and pay nothing per launch
        return 0;
    }
    *clustered = true;
    return 0;
}

// Analysis on the host (GESPMM_PLAN_ANALYSIS_HOST): the same clustering and a model of the XCD L2s that says whether the new order is
// worth having (graphs whose storage order is already local, or that have no structure to find, keep their order and pay nothing per
// launch). *clustered: cx.rp / ci / src hold the row-permuted copy for upload_host_copy.
static int order_on_host(gespmm_plan* p, Creation& cx, bool* clustered) {
    const int64_t M = p->M, K = p->K, nnz = p->nnz;
    const Stopwatch tc;
    p->perm_host.resize((size_t)M);
    const gespmm::ClusterOptions copt = cluster_options_for(p->facts, cx.threads);
    if (gespmm::cluster_rows(M, K, cx.h_rowptr.data(), cx.h_colind.data(), copt, p->perm_host.data(), &p->stats) != 0) return GESPMM_EINVAL;
    // (Moving the heavy rows to the front of each XCD slice, so that no long sequential chain starts late, was
    // measured: no effect on the community graph, 151 vs 137 us on the structureless one — hubs stay where the
    // clustering puts them, next to the rows that share their neighbours. profiles/r02/plan_hubs_first.log)
    p->cluster_seconds = tc.seconds();
    p->hits_before = gespmm::simulate_l2_hits(M, K, cx.h_rowptr.data(), cx.h_colind.data(), nullptr, 8, cx.ad.model_window, cx.ad.model_sample);
    p->hits_after = gespmm::simulate_l2_hits(M, K, cx.h_rowptr.data(), cx.h_colind.data(), p->perm_host.data(), 8, cx.ad.model_window, cx.ad.model_sample);
    if (!gespmm::keep_clustered_order(p->facts, cx.ad, p->hits_before, p->hits_after)) return 0;
    cx.rp.resize((size_t)M + 1);
    cx.ci.resize((size_t)nnz);
    cx.src.resize((size_t)M);
    cx.rp[0] = 0;
    for (int64_t i = 0; i < M; ++i) {
        const int32_t r = p->perm_host[i];
        const int32_t b = cx.h_rowptr[r], d = cx.h_rowptr[r + 1] - b;
        cx.src[i] = b;
        std::memcpy(cx.ci.data() + cx.rp[i], cx.h_colind.data() + b, (size_t)d * 4);
        cx.rp[i + 1] = cx.rp[i] + d;
    }
    *clustered = true;
    return 0;
}

// Host analysis: the task tables cut on the host (the greedy cut of device_cut_tasks), then the copy and the tables to the device.
static hipError_t upload_host_copy(gespmm_plan* p, Creation& cx, const gespmm::PlanKernelDecision& kd) {
    const int64_t M = p->M, nnz = p->nnz;
    const std::vector<int32_t>& rp = cx.rp;
    // batch-stream kernel: a task per WAVEFRONT, a row counting as at least row_floor entries; segmented-stream kernel: a task per
    // lane GROUP (its time is proportional to the entries it streams, so its tasks are cut by non-zeros alone, half the budget)
    auto cut_tasks = [&](int64_t budget, int64_t row_floor, std::vector<int32_t>& out) {
        out.reserve((size_t)(nnz / (budget > 0 ? budget : 1) + M / gespmm::kMaxRowsPerWave + 16) * 4);
        auto cost = [&](int64_t r) { return std::max<int64_t>(rp[r + 1] - rp[r], row_floor); };
        int64_t i = 0;
        while (i < M) {
            const int64_t first = i;
            int64_t acc = cost(i);
            ++i;
            while (i < M && i - first < gespmm::kMaxRowsPerWave && acc + cost(i) <= budget) {
                acc += cost(i);
                ++i;
            }
            out.push_back((int32_t)first);
            out.push_back((int32_t)(i - first));
            out.push_back(rp[first]);
            out.push_back(rp[i]);
        }
    };
    std::vector<int32_t>&tasks = cx.tasks, &gtasks = cx.gtasks;
    cut_tasks(kd.task_entries, kd.row_floor, tasks);
    cut_tasks(kd.group_task_entries, 0, gtasks);
    p->ntasks = (int32_t)(tasks.size() / 4);
    p->ngtasks = (int32_t)(gtasks.size() / 4);
    auto put = [&](void* dst, const std::vector<int32_t>& v) {
        return v.empty() ? hipSuccess : hipMemcpyAsync(dst, v.data(), v.size() * 4, hipMemcpyHostToDevice, cx.st);
    };
    hipError_t e = alloc_plan_copy(p);
    if (e == hipSuccess) e = put(p->d_rowptr, rp);
    if (e == hipSuccess) e = put(p->d_colind, cx.ci);
    if (e == hipSuccess) e = put(p->d_perm, p->perm_host);
    if (e == hipSuccess) e = put(p->d_src_begin, cx.src);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&p->d_tasks), (tasks.size() + gtasks.size()) * 4 + 16);  // (one block, as device_cut_tasks makes)
    if (e != hipSuccess) return e;
    p->d_gtasks = p->d_tasks + tasks.size();
    e = put(p->d_tasks, tasks);
    if (e == hipSuccess) e = put(p->d_gtasks, gtasks);
    return e;
}

// The plan holds its order: task tables for the two streaming kernels, the values in the plan's entry order.
static int make_task_tables(gespmm_plan* p, Creation& cx, const gespmm::PlanKernelDecision& kd) {
    hipError_t e;
    p->task_entries = kd.task_entries;
    if (cx.on_host) {
        e = upload_host_copy(p, cx, kd);
    } else {
        const int64_t budgets[2] = {kd.task_entries, kd.group_task_entries}, floors[2] = {kd.row_floor, 0};
        int32_t* tables[2] = {nullptr, nullptr};
        int32_t counts[2] = {0, 0};
        e = gespmm::device_cut_tasks(p->M, p->d_rowptr, budgets, floors, tables, counts, cx.st);
        p->d_tasks = tables[0];  // (one block holds both tables)
        p->d_gtasks = tables[1];
        p->ntasks = counts[0];
        p->ngtasks = counts[1];
        lap(cx.st, "tasks x2");
    }
    if (e == hipSuccess && p->valued && p->nnz > 0) e = permute_values(p, p->val, cx.st);
    // the caller's `val` is not read after the call returns, and the host analysis' vectors go out of scope
    if (e == hipSuccess) e = hipStreamSynchronize(cx.st);
    if (!cx.on_host) lap(cx.st, "values");
    return (int)e;
}

// Device analysis only: the tables of the staged-rows kernel (choose_plan_kernel says when: built, and kept when enough entries find
// their B row staged) and the column-slab tables (dense clustered matrices at N = 128: plan_policy.cpp slab_count_for / keep_slab_tables).
// *clustered turns false when an identity-order copy loses its reason to exist.
static int build_device_tables(gespmm_plan* p, const Creation& cx, const gespmm::PlanKernelDecision& kd, bool* clustered) {
    hipError_t e = hipSuccess;
    if (kd.build_staged) {
        e = build_staging_tables(p, cx.st);
        if (e == hipSuccess && p->stg.ev && !gespmm::keep_staged_tables(p->facts, p->stg.staged_fraction))
            gespmm::free_staging(&p->stg);  // not enough reuse inside the blocks: the streaming kernels stay
        p->staging_kept_by_policy = p->stg.ev != nullptr;
        lap(cx.st, "staging tables");
    }
    const int P = p->identity_order ? 0 : gespmm::slab_count_for(p->facts);
    if (e == hipSuccess && P >= 2) {
        e = build_slab_tables(p, P, cx.st);
        if (e == hipSuccess && p->slab.ev && !gespmm::keep_slab_tables(p->facts, p->slab.staged_fraction)) {
            gespmm::free_staging(&p->slab);
            gespmm::free_slab_view(&p->slab_view, false);
        }
        lap(cx.st, "slab tables");
    }
    if (e != hipSuccess) return (int)e;
    if (p->identity_order && !p->staging_kept_by_policy) {
        // the copy in storage order was made for the staged-rows kernel alone: without its tables the caller's arrays serve
        gespmm::free_staging(&p->stg);
        drop_plan_copy(p);
        p->identity_order = false;
        *clustered = false;
    }
    return 0;
}

// Scratch of the launches (split points / long-row partials), owned by the plan.
static int alloc_launch_scratch(gespmm_plan* p) {
    gespmm_launch_cfg cfg = {0, 0, 0, 0, 0, p->launch_flags};
    const int64_t need = gespmm_csr_spmm_workspace_bytes(p->M, p->K, p->N, p->nnz, p->variant, &cfg);
    if (need <= 0) return 0;
    const hipError_t e = hipMalloc(&p->ws, (size_t)need);
    if (e == hipSuccess) p->ws_bytes = need;
    return (int)e;
}

// Padded-record kernel (narrow widths, short rows): when asked for, or when the policy says so (plan_policy.cpp) — not beside staged
// tables that were kept.
static int build_policy_records(gespmm_plan* p, hipStream_t st) {
    if (!(gespmm::records_serves(p->M, p->K, p->N, p->max_degree) && p->nnz > 0 &&
          gespmm::want_record_tables(p->facts, p->reordered ? p->hits_after : p->hits_before) && !(p->stg.ev && p->staging_kept_by_policy)))
        return 0;
    hipError_t e = build_record_tables(p, st);
    if (e == hipErrorOutOfMemory) {  // (padding beyond the cap, or no memory: the other kernels serve the plan)
        gespmm::free_records(&p->rec);
        (void)hipGetLastError();
        e = hipSuccess;
    }
    if (e == hipSuccess && p->rec.batches && !gespmm::keep_record_tables(p->facts, record_slot_fill(p)))
        gespmm::free_records(&p->rec);  // too much padding (rows of very different lengths share tasks): the other kernels stay
    p->records_kept_by_policy = p->rec.batches != nullptr;
    return (int)e;
}

// gespmm_plan_create_v2: `opt_bytes` = sizeof(gespmm_plan_options) as the CALLER was compiled with; fields beyond it take
// their defaults, bytes beyond what this library knows are ignored (gespmm.h, "Plan options and versions").
static int plan_create_impl(gespmm_plan** out, const int32_t* rowptr, const int32_t* colind, const float* val, int64_t M,
                            int64_t K, int64_t nnz, int64_t N, int variant, const gespmm_plan_options* opt, void* stream) {
    if (!out) return GESPMM_EINVAL;
    *out = nullptr;
    int rc = check_create_args(rowptr, colind, M, K, nnz, N, variant, opt);
    if (rc != 0) return rc;
    const Stopwatch total;
    std::unique_ptr<gespmm_plan> plan(new (std::nothrow) gespmm_plan);
    gespmm_plan* p = plan.get();
    if (!p) return GESPMM_ENOMEM;
    p->M = M;
    p->K = K;
    p->nnz = nnz;
    p->N = N;
    p->variant = variant;
    p->rowptr = rowptr;
    p->colind = colind;
    p->val = val;
    p->valued = val != nullptr;
    p->analysis = opt ? opt->analysis : GESPMM_PLAN_ANALYSIS_DEVICE;
    if (const hipError_t e = hipGetDevice(&p->device)) return (int)e;
    try {
        Creation cx;
        cx.st = reinterpret_cast<hipStream_t>(stream);
        cx.on_host = p->analysis == GESPMM_PLAN_ANALYSIS_HOST;
        cx.threads = opt ? opt->threads : 0;
        if ((rc = validate_and_decide(p, cx, opt)) != 0) return rc;
        bool clustered = false;
        if (cx.ad.analyse && (rc = cx.on_host ? order_on_host(p, cx, &clustered) : order_on_device(p, cx, &clustered)) != 0) return rc;
        if (!clustered && !cx.ad.analyse && !cx.on_host && p->facts.reorder_mode == GESPMM_PLAN_NO_REORDER &&
            p->kernel_choice == GESPMM_PLAN_KERNEL_STAGED && M > 0 && nnz > 0) {
            // the caller keeps the order AND asks for the staged-rows kernel, which walks the plan's tables: the plan's copy in the identity
            // order, as for a matrix that AUTO finds already clustered (dropped again in build_device_tables where no tables come of it)
            hipError_t e = alloc_plan_copy(p);
            if (e == hipSuccess)
                e = gespmm::device_identity_copy(M, nnz, p->rowptr, p->colind, p->d_perm, p->d_rowptr, p->d_colind, p->d_src_begin, cx.st);
            if (e != hipSuccess) return (int)e;
            p->identity_order = true;
            clustered = true;
        }
        if (clustered) {
            const gespmm::PlanKernelDecision kd = gespmm::choose_plan_kernel(p->facts, p->hits_after);
            if ((rc = make_task_tables(p, cx, kd)) != 0) return rc;
            if (!cx.on_host && (rc = build_device_tables(p, cx, kd, &clustered)) != 0) return rc;
            if (clustered && kd.shallow_unroll) p->launch_flags |= GESPMM_FLAG_SHALLOW_UNROLL;
        }
        p->reordered = clustered;
        if (!clustered) p->perm_host.clear();
        if ((rc = alloc_launch_scratch(p)) != 0) return rc;
        if ((rc = build_policy_records(p, cx.st)) != 0) return rc;
    } catch (const std::bad_alloc&) {
        return GESPMM_ENOMEM;
    }
    p->analysis_seconds = total.seconds();
    if (p->reordered || p->hits_after >= 0.0) gespmm::mark_analysis_warm();  // (the analysis passes ran: their kernels are loaded now)
    *out = plan.release();
    return 0;
}

// The un-versioned entry point: every header that shipped with it alone had a gespmm_plan_options of SEVEN int32 fields
// (reorder .. analysis — round 3's 0.1 header already carried `analysis`, and this symbol honoured it), so that is what it reads;
// anything appended later is reachable through gespmm_plan_create_v2 only.
int gespmm_plan_create(gespmm_plan** out, const int32_t* rowptr, const int32_t* colind, const float* val, int64_t M,
                       int64_t K, int64_t nnz, int64_t N, int variant, const gespmm_plan_options* opt, void* stream) {
    return gespmm_plan_create_v2(out, rowptr, colind, val, M, K, nnz, N, variant, opt, opt ? 7 * (int64_t)sizeof(int32_t) : 0, stream);
}

int gespmm_plan_create_v2(gespmm_plan** out, const int32_t* rowptr, const int32_t* colind, const float* val, int64_t M,
                          int64_t K, int64_t nnz, int64_t N, int variant, const gespmm_plan_options* opt, int64_t opt_bytes,
                          void* stream) {
    if (opt && (opt_bytes < 0 || opt_bytes % 4 != 0)) return GESPMM_EINVAL;
    gespmm_plan_options o;
    std::memset(&o, 0, sizeof o);  // every field's default is 0
    if (opt && opt_bytes > 0) std::memcpy(&o, opt, (size_t)(opt_bytes < (int64_t)sizeof o ? opt_bytes : (int64_t)sizeof o));
    return plan_create_impl(out, rowptr, colind, val, M, K, nnz, N, variant, opt ? &o : nullptr, stream);
}

// The launch arguments of a set of staging tables, field by field (width, tiles and `empty` are the general kernel's launcher's to fill).
static gespmm::StagedArgs staged_args(const gespmm::StagingTables& t, const float* B, float* C, const gespmm::LaunchGuard* guard) {
    gespmm::StagedArgs a = {};
    a.ev = t.ev;
    a.tasks = t.tasks;
    a.hot_cols = t.hot_cols;
    a.B = B;
    a.C = C;
    a.nblocks = t.nblocks;
    a.waves = t.waves;
    a.slots = t.slots;
    a.guard = guard ? guard->word : nullptr;
    a.guard_want = guard ? guard->want : 0;
    return a;
}

static int plan_run(gespmm_plan* p, const float* B, float* C, int64_t N, int reduce, float empty, void* stream,
                    const gespmm::LaunchGuard* guard = nullptr) {
    using gespmm::PlanRoute;
    if (!p || N < 0) return GESPMM_EINVAL;
    if (reduce == gespmm::kReduceMax && p->valued) return GESPMM_EINVAL;
    gespmm_launch_cfg cfg = {0, 0, 0, 0, 0, p->launch_flags};
    void* ws = (N == p->N) ? p->ws : nullptr;  // another width: the library's pool serves the scratch
    const int64_t ws_bytes = (N == p->N) ? p->ws_bytes : 0;
    // the slab geometry (rows per slab) depends on the vector width the operands' alignment allows: split points kept from
    // a call with other alignment must not be reused
    const int vec_now = gespmm::vec_limit(N, gespmm::min_alignment(B, C));
    if (ws && p->split_ready && p->split_vec == vec_now) cfg.flags |= GESPMM_FLAG_REUSE_SPLIT;
    hipStream_t hst = reinterpret_cast<hipStream_t>(stream);
    const gespmm::RouteAnswer ra = route_of(p, N, reduce, aligned16(B, C));
    if (ra.route == PlanRoute::Records || ra.route == PlanRoute::StagedSlabs || ra.staged()) {  // the kernels that walk the plan's tables
        if (!B || !C) return GESPMM_EINVAL;
        if (guard && !ra.guardable()) return gespmm::kNotGuardable;  // (several launches)
        if (guard && guard->word == nullptr) return 0;               // (dry run: one kernel, guardable)
    }
    int rc = 0;
    switch (ra.route) {
    case PlanRoute::Records:
        return (int)gespmm::launch_spmm_records(p->rec, B, C, N, p->launch_flags, guard, hst);
    case PlanRoute::StagedSlabs: {
        // one launch of the staged-rows kernel per slab, the second and later ones continuing from C
        const int P = p->slab_view.slabs, nb = p->slab.nblocks / P;
        for (int s = 0; s < P && rc == 0; ++s) {
            gespmm::StagedArgs sa = staged_args(p->slab, B, C, nullptr);
            sa.nblocks = nb;  // (this slab's blocks of the tables; the second and later ones continue from C)
            sa.blk0 = s * nb;
            sa.acc = s > 0 ? 1 : 0;
            rc = (int)gespmm::launch_spmm_staged(sa, p->M, p->K, N, hst);
        }
        return rc;
    }
    case PlanRoute::StagedTuned:
    case PlanRoute::StagedNarrow:
    case PlanRoute::StagedGeneral: {
        const gespmm::StagedArgs sa = staged_args(p->stg, B, C, guard);
        if (ra.route == PlanRoute::StagedTuned) rc = (int)gespmm::launch_spmm_staged(sa, p->M, p->K, N, hst);
        else if (ra.route == PlanRoute::StagedNarrow) rc = (int)gespmm::launch_spmm_staged_narrow(sa, p->M, p->K, N, hst);
        else rc = (int)gespmm::launch_spmm_staged_gen(sa, p->M, p->K, N, reduce, empty, hst);
        if (rc == 0 && ra.hub_pass) {
            // hub rows (written as empty rows above): one-row tasks through the batch-stream kernel, whose long-row pass splits
            // them — under GESPMM_FLAG_STRICT_ORDER each is one lane group's chain instead, as everywhere else
            gespmm::CsrView hubs = plan_view(p, ra);
            hubs.variant = p->variant;
            hubs.pl = {p->stg.ltasks, p->stg.nlong, p->d_perm, nullptr, 0, false};
            gespmm_launch_cfg lcfg = cfg;
            lcfg.flags = (lcfg.flags | GESPMM_FLAG_BATCH_STREAM | GESPMM_FLAG_NO_SLAB_BLOCKED) & ~GESPMM_FLAG_REUSE_SPLIT;
            if (!(lcfg.flags & GESPMM_FLAG_STRICT_ORDER)) lcfg.flags |= GESPMM_FLAG_SPLIT_LONG_ROWS;
            rc = gespmm::run_spmm(hubs, B, C, N, &lcfg, reduce, empty, stream, ws, ws_bytes);
        }
        return rc;
    }
    case PlanRoute::PlanStream:    // the plan's copy and task tables
    case PlanRoute::StorageOrder:  // the caller's arrays
        rc = gespmm::run_spmm(plan_view(p, ra), B, C, N, &cfg, reduce, empty, stream, ws, ws_bytes, guard);
        break;
    }
    if (rc == 0 && ws) {
        p->split_ready = true;
        p->split_vec = vec_now;
    }
    return rc;
}

int gespmm_plan_spmm_f32(gespmm_plan* plan, const float* B, float* C, int64_t N, void* stream) {
    return plan_run(plan, B, C, N, gespmm::kReduceSum, 0.0f, stream);
}

int gespmm_plan_spmm_max_f32(gespmm_plan* plan, const float* B, float* C, int64_t N, float empty_value, void* stream) {
    return plan_run(plan, B, C, N, gespmm::kReduceMax, empty_value, stream);
}

// The fused product through a plan. Two executions with the same bits (plan_policy.cpp: fused_route chooses):
//   * ONE fused streaming kernel — on the caller's arrays (storage order) or on the plan's stream task tables, which every clustered
//     plan owns whatever its unfused route is (staged rows, records, slabs);
//   * the composition: col_scale . B into the plan's scratch, the plan's unfused route unchanged (plan_run), the in-place epilogue.
// `dry`: the answer only (gespmm_plan_fused_route) — operands count as 16-byte aligned, nothing is launched or allocated.
static int plan_run_fused(gespmm_plan* p, const float* B, const gespmm::FusedVectors& fx, float* C, int64_t N, void* stream, bool dry,
                          int* route_out) {
    *route_out = 0;
    const gespmm::RouteAnswer ra = route_of(p, N, gespmm::kReduceSum, dry ? true : aligned16(B, C));
    const gespmm::CsrView A = plan_view(p, ra);
    int kind = 0;
    int rc = gespmm::run_spmm_fused(A, B, fx, C, N, p->launch_flags, stream, true, &kind);
    if (rc != 0 && rc != gespmm::kFusedUnavailable) return rc;
    const int route = gespmm::fused_route(p->facts, ra, kind, N, fx.col_scale != nullptr, fx.row_scale != nullptr, fx.bias != nullptr);
    *route_out = route;
    if (dry) return 0;
    if (route != 0) return gespmm::run_spmm_fused(A, B, fx, C, N, p->launch_flags, stream, false, &kind);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const float* Bin = B;
    if (fx.col_scale && p->nnz > 0 && p->K > 0) {
        if ((rc = grow_owned(&p->d_fused_scratch, &p->fused_scratch_bytes, p->K * N * 4, st)) != 0) return rc;  // (nothing launched)
        const hipError_t e = gespmm::launch_scale_rows(B, fx.col_scale, p->d_fused_scratch, p->K, N, st);
        if (e != hipSuccess) return (int)e;
        Bin = p->d_fused_scratch;
    }
    rc = plan_run(p, Bin, C, N, gespmm::kReduceSum, 0.0f, stream);
    if (rc == 0) rc = (int)gespmm::launch_scale_bias_inplace(C, fx.row_scale, fx.bias, p->M, N, st);
    return rc;
}

int gespmm_plan_spmm_fused_f32(gespmm_plan* plan, const float* B, const float* col_scale, const float* row_scale, const float* bias,
                               float* C, int64_t N, void* stream) {
    if (!plan || N < 0) return GESPMM_EINVAL;
    const gespmm::FusedVectors fx = {col_scale, row_scale, bias};
    if (N > gespmm::kMaxWidth) return GESPMM_ERANGE;
    const bool work = plan->M > 0 && N > 0;
    if (const int rc = gespmm::check_pointers({{C, 4, work}, {B, 4, work && plan->nnz != 0}, {col_scale, 4, false}, {row_scale, 4, false}, {bias, 4, false}}))
        return rc;
    if (!work) return 0;
    if (!fx.any()) return plan_run(plan, B, C, N, gespmm::kReduceSum, 0.0f, stream);
    int route = 0;
    return plan_run_fused(plan, B, fx, C, N, stream, false, &route);
}

int gespmm_plan_fused_route(const gespmm_plan* plan, int64_t N, int has_col_scale, int has_row_scale, int has_bias) {
    if (!plan || N < 0) return GESPMM_EINVAL;
    if (plan->M == 0 || N == 0 || !(has_col_scale || has_row_scale || has_bias)) return 0;
    static const float present = 0.0f;  // (a dry run looks at which vectors are given, never at them)
    const gespmm::FusedVectors fx = {has_col_scale ? &present : nullptr, has_row_scale ? &present : nullptr, has_bias ? &present : nullptr};
    int route = 0;
    const int rc = plan_run_fused(const_cast<gespmm_plan*>(plan), nullptr, fx, nullptr, N, nullptr, true, &route);
    return gespmm::route_result(rc, route);
}

// 16-bit dense operands through a plan. Two executions with the same bits (plan_policy.cpp: x16_route chooses):
//   * ONE 16-bit streaming kernel — on the caller's arrays (storage order) or on the plan's stream task tables, which every clustered
//     plan owns whatever its fp32 route is (staged rows, records, slabs);
//   * the composition: widen(B) into the plan's temporary, the plan's fp32 route unchanged (plan_run) into a second one, narrow into C.
// `dry`: the answer only (gespmm_plan_x16_route) — nothing is launched or allocated.
static int plan_run_x16(gespmm_plan* p, const void* B, void* C, int dtype, int64_t N, void* stream, bool dry, int b_align, int c_align,
                        int* route_out) {
    *route_out = 0;
    // the streaming launch on the task tables is chosen at the byte-equivalent fp32 width, like the lane geometry (the composition's
    // fp32 route is plan_run's own business: its temporaries are aligned)
    const gespmm::CsrView A = plan_view(p, route_of(p, (N % 2 == 0 && N > 0) ? N / 2 : N, gespmm::kReduceSum, true));
    int kind = 0;
    int rc = gespmm::run_spmm_x16(A, B, C, dtype, N, p->launch_flags, stream, b_align, c_align, true, &kind);
    if (rc != 0 && rc != gespmm::kX16Unavailable) return rc;
    const int route = gespmm::x16_route(kind);
    *route_out = route;
    if (dry) return 0;
    p->x16_last_N = N;
    p->x16_last_dtype = dtype;
    if (route != 0) {
        // the launch itself looks at the stream: while it is capturing the selection drops the multi-kernel routes, so the kernel that
        // runs may be the other streaming kernel than the dry answer — what ran is what describe reports — and should the geometry
        // come out unserved the call falls through to the composition
        rc = gespmm::run_spmm_x16(A, B, C, dtype, N, p->launch_flags, stream, b_align, c_align, false, &kind, &p->x16_last_geo);
        if (rc != gespmm::kX16Unavailable) {
            p->x16_last_route = kind;
            return rc;
        }
    }
    p->x16_last_route = 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t need_b = (p->nnz != 0 && p->K > 0) ? p->K * N * 4 : 0, need_c = p->M * N * 4;
    if (p->x16_b_bytes < need_b || p->x16_c_bytes < need_c) {  // (one refusal for the pair, before either buffer is touched)
        if ((rc = gespmm::refuse_allocation_under_capture(st)) != 0) return rc;  // (nothing launched)
        hipError_t e = resize_owned(&p->d_x16_b, &p->x16_b_bytes, need_b);
        if (e == hipSuccess) e = resize_owned(&p->d_x16_c, &p->x16_c_bytes, need_c);
        if (e != hipSuccess) return (int)e;
    }
    if (need_b > 0) {
        const hipError_t e = gespmm::launch_widen_x16(B, p->d_x16_b, dtype, p->K * N, st);
        if (e != hipSuccess) return (int)e;
    }
    rc = plan_run(p, p->d_x16_b, p->d_x16_c, N, gespmm::kReduceSum, 0.0f, stream);
    if (rc == 0) rc = (int)gespmm::launch_narrow_x16(p->d_x16_c, C, dtype, p->M * N, st);
    return rc;
}

int gespmm_plan_spmm_x16(gespmm_plan* plan, const void* B, void* C, int dtype, int64_t N, void* stream) {
    if (!plan || N < 0 || !gespmm::valid_x16_dtype(dtype)) return GESPMM_EINVAL;
    if (N > gespmm::kMaxWidth) return GESPMM_ERANGE;
    const bool work = plan->M > 0 && N > 0;
    if (const int rc = gespmm::check_pointers({{C, 2, work}, {B, 2, work && plan->nnz != 0}})) return rc;
    if (!work) return 0;
    int route = 0;
    return plan_run_x16(plan, B, C, dtype, N, stream, false, gespmm::pointer_alignment(B), gespmm::pointer_alignment(C), &route);
}

int gespmm_plan_x16_route(const gespmm_plan* plan, int64_t N, int b_align, int c_align) {
    if (!plan || N < 0 || b_align < 1 || c_align < 1) return GESPMM_EINVAL;
    if (plan->M == 0 || N == 0) return 0;
    int route = 0;
    const int rc = plan_run_x16(const_cast<gespmm_plan*>(plan), nullptr, nullptr, GESPMM_X16_BF16, N, nullptr, true, b_align, c_align, &route);
    return gespmm::route_result(rc, route);
}

// The multi-head product through a plan (gespmm.h). A storage-order plan runs the stateless call on the caller's arrays. A clustered plan
// permutes the [nnz, H] weights into its own buffer (one copy kernel per call: the weights are an argument, nothing is cached) and runs the
// plan-mode heads kernel on its batch-stream task table — which every clustered plan owns whatever its scalar route is — or, where that
// kernel is not served, the stateless composition. `dry`: the answer only. `order` (may be NULL): the weights of entry e are row order[e]
// of val — a storage-order plan hands it to the stateless ordered entry, a clustered plan composes it into the copy it makes anyway.
static int plan_run_heads(gespmm_plan* p, const float* val, const float* B, float* C, int64_t H, int64_t F, void* stream, bool dry, int b_align,
                          int c_align, int* route_out, const int32_t* order = nullptr) {
    *route_out = 0;
    int kind = 0;
    gespmm::CsrView A = plan_view(p, route_of(p, H * F, gespmm::kReduceSum, true));
    if (p->reordered) {
        // (narrow_vec4 — four floats per lane at narrow widths — only where a dwordx4 stays inside one head and the operands allow it)
        if (!(F % 4 == 0 && b_align >= 16 && c_align >= 16)) A.variant = p->variant;
        A.pl = {p->d_tasks, p->ntasks, p->d_perm, nullptr, 0, false};  // the batch-stream table alone
        A.val = nullptr;                                                 // (the permuted weights: made below, once the route is known)
    } else {
        A.variant = GESPMM_VARIANT_AUTO;  // (what the stateless call below asks with)
    }
    gespmm::Geometry geo = {};
    const int rc = gespmm::run_spmm_heads(A, B, C, H, F, p->reordered ? p->launch_flags : 0, stream, b_align, c_align, true, &kind, &geo);
    if (rc != 0 && rc != gespmm::kHeadsUnavailable) return rc;
    if (p->reordered && p->d_tasks == nullptr) kind = 0;
    *route_out = kind;
    if (dry) return 0;
    p->heads_last_H = H;
    p->heads_last_F = F;
    p->heads_last_route = kind;
    if (!p->reordered) p->heads_last_geo = geo;
    if (!p->reordered || kind == 0)
        return gespmm_csr_spmm_heads_order_f32(p->rowptr, p->colind, order, val, B, C, p->M, p->K, H, F, p->nnz, stream);  // (NULL order: the plain entry)
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (const int rcg = grow_owned(&p->d_heads_val, &p->heads_val_bytes, p->nnz * H * 4, st)) return rcg;  // (nothing launched)
    const hipError_t e = gespmm::launch_permute_head_values(p->d_rowptr, p->d_src_begin, val, p->d_heads_val, p->M, p->nnz, H, st, order);
    if (e != hipSuccess) return (int)e;
    A.val = p->d_heads_val;
    return gespmm::run_spmm_heads(A, B, C, H, F, p->launch_flags, stream, b_align, c_align, false, &kind, &p->heads_last_geo);
}

int gespmm_plan_spmm_heads_f32(gespmm_plan* plan, const float* val, const float* B, float* C, int64_t H, int64_t F, void* stream) {
    if (!plan) return GESPMM_EINVAL;
    int rc = gespmm::check_heads_sizes(plan->M, plan->K, H, F, plan->nnz);
    if (rc != 0) return rc;
    if (plan->M == 0 || F == 0) return 0;
    const bool entries = plan->nnz != 0;
    if ((rc = gespmm::check_pointers({{C, 4, true}, {B, 4, entries}, {val, 4, entries}})) != 0) return rc;
    int route = 0;
    return plan_run_heads(plan, val, B, C, H, F, stream, false, gespmm::pointer_alignment(B), gespmm::pointer_alignment(C), &route);
}

int gespmm_plan_spmm_heads_order_f32(gespmm_plan* plan, const int32_t* order, const float* val, const float* B, float* C, int64_t H, int64_t F,
                                     void* stream) {
    if (!order) return gespmm_plan_spmm_heads_f32(plan, val, B, C, H, F, stream);
    if (!plan) return GESPMM_EINVAL;
    int rc = gespmm::check_heads_sizes(plan->M, plan->K, H, F, plan->nnz);
    if (rc != 0) return rc;
    if (plan->M == 0 || F == 0) return 0;
    const bool entries = plan->nnz != 0;
    if ((rc = gespmm::check_pointers({{C, 4, true}, {B, 4, entries}, {val, 4, entries}, {order, 4, false}})) != 0) return rc;
    int route = 0;
    return plan_run_heads(plan, val, B, C, H, F, stream, false, gespmm::pointer_alignment(B), gespmm::pointer_alignment(C), &route,
                          entries ? order : nullptr);
}

int gespmm_plan_heads_route(const gespmm_plan* plan, int64_t H, int64_t F, int b_align, int c_align) {
    if (!plan || b_align < 1 || c_align < 1) return GESPMM_EINVAL;
    const int rc0 = gespmm::check_heads_sizes(plan->M, plan->K, H, F, plan->nnz);
    if (rc0 != 0) return rc0;
    if (plan->M == 0 || F == 0) return 0;
    int route = 0;
    const int rc = plan_run_heads(const_cast<gespmm_plan*>(plan), nullptr, nullptr, nullptr, H, F, nullptr, true, b_align, c_align, &route);
    return gespmm::route_result(rc, route);
}

// Which kernel, MEASURED: the candidates of a clustered plan — batch-stream, segmented-stream and (at the plan's width) staged-rows —
// run on the caller's operands, `reps` launches each between a pair of events; the fastest becomes the plan's kernel. Every
// candidate produces the same bits, so C holds the product afterwards whatever wins. The static rules of plan_policy.cpp
// stay the default; this is for callers that would rather pay a few launches than trust a threshold (the hold-out audit,
// profiles/r04/holdout_audit.log, is where the rules and the measurement are compared).
namespace {
// gespmm_plan_tune's bookkeeping, settled in ONE place when the call ends: unless a winner was set, the plan leaves as it came —
// and tables do not stay behind (~16 bytes per entry, and an AUTO launch would otherwise take the staged-rows kernel against the
// policy). After a win only the winner's tables survive: launches at p->N take the winner, other widths never use the tables, and a
// later tune rebuilds them if it is asked again. After a failure only what the policy kept, or what the previous winner uses.
struct TuneScope {
    gespmm_plan* p;
    const bool was_tuned = p->tuned;
    const int was_kernel = p->tuned_kernel, was_vec = p->tuned_vec;
    bool won = false;
    explicit TuneScope(gespmm_plan* plan) : p(plan) {}
    ~TuneScope() {
        if (!won) {
            p->tuned = was_tuned;
            p->tuned_kernel = was_kernel;
            p->tuned_vec = was_vec;
        }
        auto stays = [&](int kernel, bool kept_by_policy) {
            return won ? p->tuned_kernel == kernel : (kept_by_policy || (was_tuned && was_kernel == kernel));
        };
        if (!stays(GESPMM_PLAN_KERNEL_STAGED, p->staging_kept_by_policy)) {
            gespmm::free_staging(&p->stg);
            p->staging_kept_by_policy = false;
        }
        if (!stays(GESPMM_PLAN_KERNEL_RECORDS, p->records_kept_by_policy)) {
            gespmm::free_records(&p->rec);
            p->records_kept_by_policy = false;
        }
    }
};
}  // namespace

int gespmm_plan_tune(gespmm_plan* p, const float* B, float* C, int64_t N, int32_t reps, void* stream) {
    using gespmm::PlanRoute;
    if (!p || N <= 0 || !B || !C) return GESPMM_EINVAL;
    if (N != p->N) return GESPMM_EINVAL;  // the tables are made for one width
    // a storage-order plan has one launch path, and the caller's explicit choice stands: nothing to measure, but C = A * B as promised
    // (... and so does a plan that kept column-slab tables: they are not one of the candidates below, and the rule that kept them —
    //  half of the entries staged on a matrix of mean degree >= 96 — is far from the margin: x0.73-0.81 wherever it fires, slab_density.log)
    if (!p->reordered || p->kernel_choice != GESPMM_PLAN_KERNEL_AUTO || p->slab.ev)
        return plan_run(p, B, C, N, gespmm::kReduceSum, 0.0f, stream);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (gespmm::is_capturing(st)) return GESPMM_EINVAL;
    if (reps <= 0) reps = 3;
    if (reps > 50) reps = 50;
    TuneScope scope(p);
    // tables built for the occasion: kept only if their kernel wins
    const bool v4 = gespmm::variant_takes_vec4(p->variant);
    if (!p->stg.ev && p->analysis == GESPMM_PLAN_ANALYSIS_DEVICE && v4 && p->nnz > 0 && gespmm::staged_serves_any(p->M, p->K, p->N) &&
        gespmm::staged_stream_fits(p->M, p->nnz)) {
        const hipError_t e = build_staging_tables(p, st);
        if (e != hipSuccess) return (int)e;
    }
    if (!p->rec.batches && v4 && p->nnz > 0 && gespmm::records_serves(p->M, p->K, p->N, p->max_degree) && build_record_tables(p, st) != hipSuccess) {
        gespmm::free_records(&p->rec);  // (the other candidates are measured without)
        (void)hipGetLastError();
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = (int)hipEventCreate(&e0);
    if (rc == 0) rc = (int)hipEventCreate(&e1);
    const int cand[5] = {GESPMM_PLAN_KERNEL_STREAM, GESPMM_PLAN_KERNEL_SEG_STREAM, GESPMM_PLAN_KERNEL_STAGED, GESPMM_PLAN_KERNEL_STREAM,
                         GESPMM_PLAN_KERNEL_RECORDS};
    int best = -1;
    p->tuned = true;  // (plan_run below launches the candidate through the tuned path)
    for (int c = 0; c < 5 && rc == 0; ++c) {
        p->tune_us[c] = -1.0;
        p->tuned_kernel = cand[c];
        p->tuned_vec = c == 3 ? 1 : 0;
        // is the candidate what a launch would take? (plan_route takes the tuned lane geometry as given: whether four floats per lane
        // exist at this width is asked here.) Asking the route is stricter than asking whether the tables exist: tables that no kernel
        // would walk at this width, block shape or variant are skipped instead of timing the streaming kernel under their name — the
        // table builders make no such tables, so no plan they can produce is measured differently.
        const gespmm::RouteAnswer ra = route_of(p, N, gespmm::kReduceSum, aligned16(B, C));
        const bool available = c == 1   ? ra.route == PlanRoute::PlanStream && ra.segmented
                               : c == 2 ? ra.staged()
                               : c == 3 ? p->variant == GESPMM_VARIANT_AUTO && N <= 64 && N % 4 == 0
                               : c == 4 ? ra.route == PlanRoute::Records
                                        : true;
        if (!available) continue;
        rc = plan_run(p, B, C, N, gespmm::kReduceSum, 0.0f, stream);  // warm: code objects, split points, L2 state
        if (rc == 0) rc = (int)hipEventRecord(e0, st);
        for (int r = 0; r < reps && rc == 0; ++r) rc = plan_run(p, B, C, N, gespmm::kReduceSum, 0.0f, stream);
        if (rc == 0) rc = (int)hipEventRecord(e1, st);
        if (rc == 0) rc = (int)hipEventSynchronize(e1);
        float ms = 0.0f;
        if (rc == 0) rc = (int)hipEventElapsedTime(&ms, e0, e1);
        if (rc != 0) break;
        p->tune_us[c] = (double)ms * 1e3 / reps;
        if (best < 0 || p->tune_us[c] < p->tune_us[best]) best = c;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (rc != 0 || best < 0) return rc;  // a candidate failed: the plan is what it was before the call (TuneScope)
    p->tuned_kernel = cand[best];
    p->tuned_vec = best == 3 ? 1 : 0;
    scope.won = true;
    if (best != 2) rc = plan_run(p, B, C, N, gespmm::kReduceSum, 0.0f, stream);  // (C is the winner's product either way: same bits)
    return rc;
}

// The buffers a plan keeps for SDDMM, each made by the first call that needs it (gespmm_plan_sddmm_* and gespmm_plan_sddmm_heads_f32).
// Route 1: the row id of every edge of the caller's CSR, expanded once.
static hipError_t plan_sddmm_row_ids(gespmm_plan* p, hipStream_t st) {
    if (p->d_coo_row_storage) return hipSuccess;
    int32_t* rows = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&rows), (size_t)p->nnz * 4);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(expand_rows_kernel, dim3((unsigned)((p->nnz + 255) / 256)), dim3(256), 0, st, p->rowptr, rows, (int)p->M, (int)p->nnz);
    e = hipGetLastError();
    if (e != hipSuccess) {
        (void)hipFree(rows);
        return e;
    }
    p->d_coo_row_storage = rows;
    return hipSuccess;
}

// Route 2: row ids and destinations of the edges in the plan's clustered order, and the nnz temporary the results pass through.
static hipError_t plan_sddmm_edge_maps(gespmm_plan* p, hipStream_t st) {
    if (p->d_coo_row) return hipSuccess;
    const size_t bytes = (size_t)p->nnz * 4;
    // all three buffers or none: a half-built set must not survive into the next call
    int32_t *coo = nullptr, *dst = nullptr;
    float* tmp = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&coo), bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&dst), bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&tmp), bytes);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(plan_edge_maps_kernel, dim3((unsigned)((p->nnz + 255) / 256)), dim3(256), 0, st, p->d_rowptr, p->d_src_begin,
                           p->d_perm, coo, dst, (int)p->M, (int)p->nnz);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        if (coo) (void)hipFree(coo);
        if (dst) (void)hipFree(dst);
        if (tmp) (void)hipFree(tmp);
        return e;
    }
    p->d_coo_row = coo;
    p->d_edge_dst = dst;
    p->d_sddmm_tmp = tmp;
    return hipSuccess;
}

// SDDMM on the plan's pattern: out[e] = <D1[row(e), :], D2[col(e), :]> for every edge e of the CALLER's CSR (out in the
// caller's edge order). A clustered plan walks the edges in its own order — the rows of D2 that neighbouring rows share
// are then found in L2, as in the SpMM — and scatters the results back; each dot product is the same lane butterfly as in
// gespmm_sddmm_{coo,csr}_f32, so the bits are the same.
// dtype: 0 fp32 operands, GESPMM_X16_F16 / GESPMM_X16_BF16 16-bit ones (gespmm_plan_sddmm_x16) — the routes, the buffers the plan keeps for
// them (row ids, edge maps, the fp32 temporary: `out` is fp32 either way) and the order of the checks are the same.
static int plan_sddmm(gespmm_plan* p, const void* D1, const void* D2, float* out, int dtype, int64_t N, void* stream) {
    // the checks of gespmm_sddmm_{coo,csr}_{f32,x16}, in their order (routes 1 and 2 launch without passing through them)
    if (!p || N < 0) return GESPMM_EINVAL;
    if (dtype != 0 && !gespmm::valid_x16_dtype(dtype)) return GESPMM_EINVAL;
    if (N > gespmm::kMaxWidth || p->nnz > gespmm::kSddmmMaxNnz) return GESPMM_ERANGE;
    if (p->nnz == 0) return 0;
    const int elem = dtype == 0 ? 4 : 2;
    if (const int rc = gespmm::check_pointers({{out, 4, true}, {D1, elem, N > 0}, {D2, elem, N > 0}})) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // the one launch all three routes make: the stateless library's, for the operand type
    auto launch = [&](const int32_t* rows, bool csr, const int32_t* cols, float* dst) {
        if (dtype == 0)
            return gespmm::launch_sddmm(rows, csr, cols, static_cast<const float*>(D1), static_cast<const float*>(D2), dst, p->M, p->nnz, N, st);
        return gespmm::launch_sddmm_x16(rows, csr, cols, D1, D2, dst, dtype, p->M, p->nnz, N, st);
    };
    // which form: sddmm_route (plan_policy.cpp) — 0 CSR call, 1 COO on row ids expanded ONCE (same lane butterfly per edge, same
    // bits), 2 the plan's clustered edge order + scatter
    hipError_t e = hipSuccess;
    const int route = gespmm::sddmm_route(p->facts, p->reordered, p->hits_after, N);
    if (route != 2) {
        if (route == 1) {
            e = plan_sddmm_row_ids(p, st);
            if (e != hipSuccess) return (int)e;
            return (int)launch(p->d_coo_row_storage, false, p->colind, out);
        }
        if (dtype == 0) return gespmm_sddmm_csr_f32(p->rowptr, p->colind, static_cast<const float*>(D1), static_cast<const float*>(D2), out, p->M, p->nnz, N, stream);
        return gespmm_sddmm_csr_x16(p->rowptr, p->colind, D1, D2, out, dtype, p->M, p->nnz, N, stream);
    }
    e = plan_sddmm_edge_maps(p, st);
    if (e != hipSuccess) return (int)e;
    e = launch(p->d_coo_row, false, p->d_colind, p->d_sddmm_tmp);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(scatter_by_index_kernel, dim3((unsigned)((p->nnz + 255) / 256)), dim3(256), 0, st, p->d_sddmm_tmp,
                       p->d_edge_dst, out, (int)p->nnz);
    return (int)hipGetLastError();
}

int gespmm_plan_sddmm_f32(gespmm_plan* p, const float* D1, const float* D2, float* out, int64_t N, void* stream) {
    return plan_sddmm(p, D1, D2, out, 0, N, stream);
}

int gespmm_plan_sddmm_x16(gespmm_plan* p, const void* D1, const void* D2, float* out, int dtype, int64_t N, void* stream) {
    if (!gespmm::valid_x16_dtype(dtype)) return GESPMM_EINVAL;
    return plan_sddmm(p, D1, D2, out, dtype, N, stream);
}

int gespmm_plan_sddmm_route(const gespmm_plan* p, int64_t N) {
    if (!p || N < 0) return GESPMM_EINVAL;
    return gespmm::sddmm_route(p->facts, p->reordered, p->hits_after, N);
}

// The multi-head SDDMM on the plan's pattern (gespmm.h): out[e H + h] in the caller's CSR edge order, the bits of gespmm_sddmm_csr_heads_f32.
// The routes are plan_sddmm's, decided by the same rule at the width of the gathered row, H F; a pair count past the heads kernel's
// limit leaves only the stateless call (its composition).
static int plan_sddmm_heads_route(const gespmm_plan* p, int64_t H, int64_t F) {
    if (p->nnz > gespmm::kSddmmMaxNnz / H) return 0;
    return gespmm::sddmm_route(p->facts, p->reordered, p->hits_after, H * F);
}

int gespmm_plan_sddmm_heads_f32(gespmm_plan* p, const float* D1, const float* D2, float* out, int64_t H, int64_t F, void* stream) {
    if (!p) return GESPMM_EINVAL;
    const int rc0 = gespmm::check_sddmm_heads_sizes(true, p->M, H, F, p->nnz);
    if (rc0 != 0) return rc0;
    if (p->nnz == 0) return 0;
    if (const int rc = gespmm::check_pointers({{out, 4, true}, {D1, 4, F > 0}, {D2, 4, F > 0}})) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int route = F == 0 ? 0 : plan_sddmm_heads_route(p, H, F);
    if (route == 0) return gespmm::run_sddmm_heads(p->rowptr, true, p->colind, D1, D2, out, p->M, p->K, H, F, p->nnz, stream);
    if (route == 1) {
        const hipError_t e = plan_sddmm_row_ids(p, st);
        if (e != hipSuccess) return (int)e;
        return gespmm::run_sddmm_heads(p->d_coo_row_storage, false, p->colind, D1, D2, out, p->M, p->K, H, F, p->nnz, stream);
    }
    hipError_t e = plan_sddmm_edge_maps(p, st);
    if (e != hipSuccess) return (int)e;
    if (const int rcg = grow_owned(&p->d_sddmm_heads_tmp, &p->sddmm_heads_tmp_bytes, p->nnz * H * 4, st)) return rcg;  // (nothing launched)
    const int rc = gespmm::run_sddmm_heads(p->d_coo_row, false, p->d_colind, D1, D2, p->d_sddmm_heads_tmp, p->M, p->K, H, F, p->nnz, stream);
    if (rc != 0) return rc;
    return (int)gespmm::launch_scatter_heads(p->d_sddmm_heads_tmp, p->d_edge_dst, out, p->nnz, H, st);
}

int gespmm_plan_sddmm_heads_route(const gespmm_plan* p, int64_t H, int64_t F) {
    if (!p) return GESPMM_EINVAL;
    const int rc = gespmm::check_sddmm_heads_sizes(true, p->M, H, F, p->nnz);
    if (rc != 0) return rc;
    return plan_sddmm_heads_route(p, H, F);
}

int gespmm_plan_set_values(gespmm_plan* p, const float* val, void* stream) {
    if (!p) return GESPMM_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (!p->reordered) {
        p->val = val;
        p->valued = val != nullptr;
        if (p->rec.batches) return (int)gespmm::device_records_set_values(p->rec, p->M, p->rowptr, p->colind, val, st);
        return 0;
    }
    if (!val) {
        p->valued = false;
        if (p->rec.batches) {
            const hipError_t er = gespmm::device_records_set_values(p->rec, p->M, p->d_rowptr, p->d_colind, nullptr, st);
            if (er != hipSuccess) return (int)er;
        }
        if (p->slab.ev) {
            const hipError_t es = gespmm::device_slab_set_values(p->slab, p->slab_view, nullptr, p->M * p->slab_view.slabs, p->nnz, st);
            if (es != hipSuccess) return (int)es;
        }
        if (p->stg.ev) return (int)gespmm::device_staging_set_values(p->stg, nullptr, p->d_rowptr, p->M, p->nnz, st);  // the stream carries 1.0f
        return 0;
    }
    if (!p->d_val) {  // (created without values: the plan's block has no room for them)
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p->d_val_late), (size_t)(p->nnz > 0 ? p->nnz : 1) * 4);
        if (e != hipSuccess) return (int)e;
        p->d_val = p->d_val_late;
    }
    p->valued = true;
    if (p->nnz == 0) return 0;
    const hipError_t ep = permute_values(p, val, st);
    if (ep != hipSuccess) return (int)ep;
    if (p->stg.ev) {
        const hipError_t es = gespmm::device_staging_set_values(p->stg, p->d_val, p->d_rowptr, p->M, p->nnz, st);
        if (es != hipSuccess) return (int)es;
    }
    if (p->slab.ev) {
        const hipError_t es = gespmm::device_slab_set_values(p->slab, p->slab_view, p->d_val, p->M * p->slab_view.slabs, p->nnz, st);
        if (es != hipSuccess) return (int)es;
    }
    if (p->rec.batches) {
        const hipError_t er = gespmm::device_records_set_values(p->rec, p->M, p->d_rowptr, p->d_colind, p->d_val, st);
        if (er != hipSuccess) return (int)er;
    }
    return (int)hipGetLastError();
}

int gespmm_plan_get_order(const gespmm_plan* p, int32_t* perm_host) {
    if (!p || (p->M > 0 && !perm_host)) return GESPMM_EINVAL;
    if (p->reordered && p->perm_host.size() != (size_t)p->M) {  // device analysis: the order lives on the device
        if (hipMemcpy(perm_host, p->d_perm, (size_t)p->M * 4, hipMemcpyDeviceToHost) != hipSuccess) return GESPMM_EINVAL;
    } else if (p->reordered) std::memcpy(perm_host, p->perm_host.data(), (size_t)p->M * 4);
    else
        for (int64_t i = 0; i < p->M; ++i) perm_host[i] = (int32_t)i;
    return p->reordered ? 1 : 0;
}

int gespmm_plan_describe(const gespmm_plan* p, char* out, int64_t capacity) {
    using gespmm::PlanRoute;
    if (!p || !out || capacity <= 0) return GESPMM_EINVAL;
    // what a sum launch at the plan's own width does on 16-byte operands: the answer plan_run acts on
    const gespmm::RouteAnswer ra = route_of(p, p->N, gespmm::kReduceSum, true);
    char what[256] = "";  // the streaming launch (of that width too: what the max reducer and unaligned operands get)
    gespmm_launch_cfg cfg = {0, 0, 0, 0, 0, p->launch_flags | (p->reordered ? ((ra.segmented ? GESPMM_FLAG_SEG_STREAM : GESPMM_FLAG_BATCH_STREAM) | GESPMM_FLAG_NO_SLAB_BLOCKED) : 0)};
    gespmm_describe_launch(p->M, p->K, p->N, p->nnz, ra.vec4 ? GESPMM_VARIANT_CRC_CWM4 : p->variant, &cfg, what, sizeof what);
    char kern[520];
    if (ra.route == PlanRoute::Records)
        snprintf(kern, sizeof kern, "kernel=padded-records tasks=%d batches_per_task>=%d batches=%d slot_fill=%.3f tables=%.4fs (max / other widths: %s)",
                 p->rec.ntasks, p->rec.target_batches, p->rec.nbatches, record_slot_fill(p), p->records_seconds, what);
    else if (ra.route == PlanRoute::StagedSlabs)
        snprintf(kern, sizeof kern, "kernel=staged-slabs slabs=%d blocks=%d rows_in_lds<=%d staged_entries=%.3f tables=%.4fs (max / other widths: %s)",
                 p->slab_view.slabs, p->slab.nblocks, p->slab.slots, p->slab.staged_fraction, p->slab_seconds, what);
    else if (ra.staged())
        snprintf(kern, sizeof kern, "kernel=staged-rows blocks=%d rows_in_lds<=%d staged_entries=%.3f filled_entries=%.3f hub_rows=%d tables=%.4fs (max / other widths: %s)",
                 p->stg.nblocks, gespmm::staged_block_shape(p->N).slots, p->stg.staged_fraction, p->stg.filled_fraction, p->stg.nlong, p->staging_seconds, what);
    else snprintf(kern, sizeof kern, "%s", what);
    if (p->x16_last_route >= 0) {  // the last 16-bit call (gespmm_plan_spmm_x16)
        const size_t used = strlen(kern);
        char geo[64] = "";
        if (p->x16_last_route != 0)
            snprintf(geo, sizeof geo, " V=%d S=%d W=%d", p->x16_last_geo.vec, p->x16_last_geo.strips, p->x16_last_geo.group);
        snprintf(kern + used, sizeof kern - used, " | x16 %s N=%lld route=%d (%s%s)", p->x16_last_dtype == GESPMM_X16_F16 ? "f16" : "bf16",
                 (long long)p->x16_last_N, p->x16_last_route,
                 p->x16_last_route == 1 ? "16-bit batch-stream" : p->x16_last_route == 2 ? "16-bit segmented-stream" : "widen, fp32 route, narrow",
                 geo);
    }
    if (p->heads_last_route >= 0) {  // the last multi-head call (gespmm_plan_spmm_heads_f32)
        const size_t used = strlen(kern);
        char geo[64] = "";
        if (p->heads_last_route != 0)
            snprintf(geo, sizeof geo, " V=%d S=%d W=%d", p->heads_last_geo.vec, p->heads_last_geo.strips, p->heads_last_geo.group);
        snprintf(kern + used, sizeof kern - used, " | heads H=%lld F=%lld route=%d (%s%s)", (long long)p->heads_last_H, (long long)p->heads_last_F,
                 p->heads_last_route, p->heads_last_route == 1 ? (p->reordered ? "heads kernel, task table" : "heads kernel") : "per-head composition",
                 geo);
    }
    int n;
    if (p->reordered) {
        char lv[128] = "";
        int off = 0;
        for (int i = 0; i < p->stats.levels && i < 16 && off < 100; ++i)
            off += snprintf(lv + off, sizeof lv - (size_t)off, "%s%d", i ? ">" : "", p->stats.clusters[i]);
        char tuned[200] = "";
        if (p->tuned)
            snprintf(tuned, sizeof tuned, " tuned[us: batch-stream=%.1f segmented-stream=%.1f staged-rows=%.1f batch-stream-V4=%.1f padded-records=%.1f]",
                     p->tune_us[0], p->tune_us[1], p->tune_us[2], p->tune_us[3], p->tune_us[4]);
        n = snprintf(out, (size_t)capacity,
                     "order=%s levels=%d clusters=%s tasks=%d task_entries=%d group_tasks=%d max_degree=%d probe=%.3f l2_model=%.3f->%.3f "
                     "analysis=%.4fs on the %s (clustering %.4fs)%s | %s",
                     p->identity_order ? "storage(plan copy: as local as the clustering)" : "clustered", p->stats.levels, lv, p->ntasks, p->task_entries,
                     p->ngtasks, p->max_degree, p->facts.wedge_probe, p->hits_before,
                     p->hits_after, p->analysis_seconds, p->analysis == GESPMM_PLAN_ANALYSIS_HOST ? "host" : "device", p->cluster_seconds, tuned, kern);
    } else {
        char why[200] = "";
        if (p->cost_skipped)
            snprintf(why, sizeof why, " (analysis skipped: est. gain %.1f us x %d launches < est. cost %.0f us; wedge probe %.4f)", p->est_gain_us,
                     p->facts.expected_launches > 0 ? p->facts.expected_launches : gespmm::kDefaultExpectedLaunches, p->est_cost_us,
                     p->facts.wedge_probe);
        n = snprintf(out, (size_t)capacity, "order=storage max_degree=%d l2_model=%.3f->%.3f analysis=%.4fs%s | %s",
                     p->max_degree, p->hits_before, p->hits_after, p->analysis_seconds, why, kern);
    }
    return gespmm::describe_result(n, capacity);
}

void gespmm_release_cached_memory(void) { gespmm::release_cached_arena(); }

void gespmm_set_cached_memory_limit(int64_t bytes) { gespmm::set_arena_cache_limit((long long)bytes); }

void gespmm_plan_destroy(gespmm_plan* p) { delete p; }

}  // extern "C"

namespace gespmm {
int plan_spmm_guarded(gespmm_plan* plan, const float* B, float* C, int64_t N, int reduce, float empty, void* stream, const LaunchGuard* guard) {
    return plan_run(plan, B, C, N, reduce, empty, stream, guard);
}
}  // namespace gespmm
