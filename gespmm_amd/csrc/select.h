// select.h — host-only variant / launch-geometry selection (no HIP calls).
#pragma once
#include <stdint.h>

#include "spmm_kernels.h"

namespace gespmm {

struct Selection {
    int variant;   // resolved GESPMM_VARIANT_* (never AUTO)
    Geometry geo;
};

// What GESPMM_VARIANT_AUTO resolves to. Only bit-exact variants (0-4) are ever
// chosen automatically; the parallel-reduction variant is opt-in.
int auto_variant(int64_t M, int64_t nnz, int64_t N);

// Fill `out` for (shape, variant, optional overrides). max_vec is the widest
// vector the pointers/N allow (1, 2 or 4). Returns 0 or a GESPMM_E* code.
int resolve_geometry(int64_t M, int64_t K, int64_t N, int64_t nnz, int variant, int max_vec,
                     int cfg_vec, int cfg_strips, int cfg_group, int cfg_rows_per_wave, int cfg_slab_rows, int flags,
                     Selection* out);

// ---- SDDMM: which of its four launch forms a call takes (launch_sddmm runs exactly this; gespmm_describe_sddmm prints it).
enum SddmmForm {
    kSddmmCooEdge = 0,  // edge-parallel kernel on the caller's row ids
    kSddmmCsrEdge = 1,  // edge-parallel kernel, rows found through an LDS window of row pointers (epw edges per wavefront)
    kSddmmRowWalk = 2,  // a row per wavefront over the whole row (mean degree >= 64)
    kSddmmBlocked = 3,  // the row-walking kernel once per ~6 MB column slab of D2 (allocates: never while capturing)
};
struct SddmmLaunch {
    int form;           // SddmmForm
    int V, W;           // elements per load, lanes per edge: these two fix the summation order
    int epw;            // edges per wavefront of the edge-parallel forms (0 for the row-walking ones)
    int64_t nslab;      // blocked form: launches; else 0
    int64_t slab_rows;  // blocked form: D2 rows per slab; else 0
};
// d1_align / d2_align: largest power of two (bytes) that divides the operand's address, 16 is as good as more.
// elem_size: bytes per element of D1 / D2 — 4 (fp32) or 2 (fp16 / bf16: V up to 8, every byte threshold at half the width).
SddmmLaunch resolve_sddmm(bool csr, int64_t M, int64_t nnz, int64_t N, int d1_align, int d2_align, bool capturing, int elem_size = 4);

// ---- multi-head SDDMM (sddmm_heads.h): which route a call takes and, for the kernel, its launch shape (run_sddmm_heads runs exactly
// this; gespmm_describe_sddmm_heads prints it).
enum SddmmHeadsRoute {
    kSddmmHeadsComposition = 0,  // per head: slices of D1 and D2, launch_sddmm at width F, scatter into out[:, h] (allocates)
    kSddmmHeadsKernel = 1,       // ONE sddmm_heads_kernel (never allocates)
    kSddmmHeadsPlain = 2,        // H == 1: the single-head call on the caller's arrays
};
enum SddmmHeadsPin { kSddmmHeadsPinNone = 0, kSddmmHeadsPinKernel = 1, kSddmmHeadsPinComposition = 2 };
struct SddmmHeadsLaunch {
    int route;       // SddmmHeadsRoute
    int form;        // kernel: kSddmmCooEdge or kSddmmCsrEdge; else the form resolve_sddmm answers at width F
    int V, W;        // what resolve_sddmm answers for WIDTH F and the two operand addresses: they fix the bits of every route
    int epw;         // kernel: EDGES per wavefront, 1 .. 256 (epw H pairs); else 0
    uint32_t magic;  // kernel: ceil(2^32 / H) where t / H == umulhi(t, magic) for every t < 256 H, else 0 (the kernel divides)
};
// pin: GESPMM_SDDMM_HEADS_ROUTE of the caller (kernel: ignored where the kernel cannot run; composition: CSR form off a capturing
// stream only). nnz > 0, H >= 1. elem_size: bytes per element of D1 / D2, as resolve_sddmm's (2: V up to 8).
SddmmHeadsLaunch resolve_sddmm_heads(bool csr, int64_t M, int64_t nnz, int64_t H, int64_t F, int d1_align, int d2_align, bool capturing,
                                     int pin = kSddmmHeadsPinNone, int elem_size = 4);

// ---- edge softmax (edge_softmax.h): the launch shape of forward and backward alike (gespmm_describe_edge_softmax prints W and L).
constexpr int kEdgeSoftmaxIT = 4;                                // entries per lane a row may have to be read once (registers)
constexpr int kEdgeSoftmaxMaxW = 16;                             // most lanes per pair of a row of at most L entries (measured: select.cpp)
constexpr int64_t kEdgeSoftmaxMaxRows = 0x7fffffffLL - 4096;     // row ids of the last workgroup's wavefronts stay below 2^31
struct EdgeSoftmaxLaunch {
    int W;    // lanes per (row, head) pair of a row of at most L entries: smallest power of two >= ceil(nnz / M), within [4, 16]
    int L;    // rows of more entries take a whole wavefront per pair, W = 64 (kLongRowThreshold)
    int rpw;  // rows per wavefront, 1 .. 63: about 64 pairs (one row where H >= 64). Never changes a bit of the result.
};
// M >= 1, nnz >= 1, H >= 1. W and L depend on (M, nnz) alone.
EdgeSoftmaxLaunch resolve_edge_softmax(int64_t M, int64_t nnz, int64_t H);

// ---- GATv2 edge score (gatv2_score.h): the launch shape of the forward (gespmm_describe_gatv2_score prints it).
struct Gatv2ScoreLaunch {
    int V, W;        // what resolve_sddmm answers for WIDTH F, with att's address as a third operand: they fix the summation order
    int epw;         // ENTRIES per wavefront, 1 .. 256 (epw H pairs)
    uint32_t magic;  // ceil(2^32 / H) where t / H == umulhi(t, magic) for every t < 256 H, else 0 (the kernel divides)
};
// nnz >= 1, H >= 1, F >= 1. *_align: largest power of two (bytes) that divides the operand's address, 16 is as good as more.
Gatv2ScoreLaunch resolve_gatv2_score(int64_t M, int64_t nnz, int64_t H, int64_t F, int xl_align, int xr_align, int att_align);
// The same for fp16 / bf16 xl and xr with an fp32 att (gespmm_describe_gatv2_score_x16 prints it): V counts ELEMENTS, 8 / 4 / 2 / 1 — V
// divides F, 2 V bytes divide the addresses of xl and xr, min(4 V, 16) bytes divide att's. xl_align, xr_align >= 2, att_align >= 4.
Gatv2ScoreLaunch resolve_gatv2_score_x16(int64_t M, int64_t nnz, int64_t H, int64_t F, int xl_align, int xr_align, int att_align);

// ---- fused dot-product attention (dot_attention.h): the lane geometry of its three kernels (gespmm_describe_dot_attention prints it).
constexpr int64_t kDotAttentionMaxF = 512;  // a lane holds 8 floats of a head slice, a lane group has at most 64 lanes
struct DotAttentionLaunch {
    int V, W;        // what resolve_sddmm answers for WIDTH F and the least aligned dense operand: they fix the dot's summation order
    bool supported;  // F <= kDotAttentionMaxF; false: no kernel serves the shape, V and W mean nothing
};
// F >= 1. *_align: largest power of two (bytes) that divides an operand's address — the least of a launch's dense operands decides.
DotAttentionLaunch resolve_dot_attention(int64_t F, int q_align, int k_align, int v_align);
// ... on 16-bit node terms (dot_attention_x16.h): V counts ELEMENTS and stays in {4, 2, 1} — 2 V bytes divide every alignment (the least
// of the 16-bit operands and results, >= 2). The answer is resolve_dot_attention's at twice each alignment, capped at 16: a 16-bit
// operand b bytes off a 16-byte boundary is an fp32 operand 2 b bytes off.
DotAttentionLaunch resolve_dot_attention_x16(int64_t F, int q_align, int k_align, int v_align);

// ---- fused GATv2 attention (gatv2_attention.h): the lane geometry of its three kernels (gespmm_describe_gatv2_attention prints it).
constexpr int64_t kGatv2AttentionMaxF = 512;  // a lane holds 8 floats of a head slice, a lane group has at most 64 lanes
struct Gatv2AttentionLaunch {
    int V, W;        // what resolve_sddmm answers for WIDTH F and the least aligned dense operand: they fix the score's summation order
    bool supported;  // F <= kGatv2AttentionMaxF; false: no kernel serves the shape, V and W mean nothing
};
// F >= 1. *_align: largest power of two (bytes) that divides an operand's address — the least of a launch's dense operands decides.
Gatv2AttentionLaunch resolve_gatv2_attention(int64_t F, int xl_align, int xr_align, int att_align);
// ... on 16-bit node terms (gatv2_attention_x16.h): V counts ELEMENTS and stays in {4, 2, 1} — 2 V bytes divide xl_align and xr_align
// (the least of the 16-bit operands and results, >= 2), 4 V bytes divide att_align (the least of att and att_part, >= 4). The answer is
// resolve_gatv2_attention's for the widened operands: a 16-bit operand b bytes off a 16-byte boundary is an fp32 operand 2 b bytes off.
Gatv2AttentionLaunch resolve_gatv2_attention_x16(int64_t F, int xl_align, int xr_align, int att_align);

}  // namespace gespmm
