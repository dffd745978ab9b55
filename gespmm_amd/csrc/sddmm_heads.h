// sddmm_heads.h — the MULTI-HEAD SDDMM (gespmm_sddmm_{coo,csr}_heads_f32: instantiated for fp32 in sddmm_heads.hip;
// gespmm_sddmm_{coo,csr}_heads_x16: for fp16 / bf16 operands, on the trait SddmmX16<DT>, in sddmm_x16.hip).
//
// D1 is [M, H F], D2 is [K, H F], out is [nnz, H], all row-major, and
//   out[e H + h] = dot_{V,W}( D1[row(e), h F : (h + 1) F], D2[col(e), h F : (h + 1) F] )
// where dot_{V,W} is the summation order sddmm_edge.h pins — lane l of W runs one fmaf chain over j = l V + i + t W V, then an xor
// butterfly with masks W/2 .. 1 — at the (V, W) resolve_sddmm answers for WIDTH F and the operands' element size. V counts elements,
// divides F, and V elements' bytes (4 V; 16-bit operands: 2 V, V up to 8) divide both base addresses, so every head slice of every row is a legal V-vector address and no vector spans two heads: head h has the bits of the
// single-head product on D1[:, hF:(h+1)F] and D2[:, hF:(h+1)F], whatever H, the form or the route.
//
// The kernel is the edge-parallel kernel of sddmm_edge.h with the (edge, head) PAIR q = e H + h as the unit of work: a wavefront owns
// epw consecutive edges — epw H consecutive pairs, stored to consecutive words of out — and in CSR form resolves the row and column of
// each of its edges ONCE (one wavefront-wide row search, the row-pointer window in LDS) for all H heads. H and F are run-time values;
// LDS is sized by edges, so H is unbounded. resolve_sddmm_heads (select.cpp) decides route, form, V, W and epw; launch_sddmm_heads runs
// exactly what it answers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "select.h"

namespace gespmm {

// r.route == kSddmmHeadsKernel. rows: row ids (r.form == kSddmmCooEdge) or row pointers (kSddmmCsrEdge). nnz H <= kSddmmMaxNnz, F >= 1.
hipError_t launch_sddmm_heads(const int32_t* rows, const int32_t* colind, const float* D1, const float* D2, float* out, int64_t M,
                              int64_t nnz, int64_t H, int64_t F, const SddmmHeadsLaunch& r, hipStream_t st);
// The same on 16-bit operands (dtype kX16F16 / kX16Bf16; out stays fp32): r is resolve_sddmm_heads' answer at element size 2.
hipError_t launch_sddmm_heads_x16(const int32_t* rows, const int32_t* colind, const void* D1, const void* D2, float* out, int dtype,
                                  int64_t M, int64_t nnz, int64_t H, int64_t F, const SddmmHeadsLaunch& r, hipStream_t st);
// *result = max(0, max_i idx[i]) — the composition route's bound on the rows of D2 a CSR call touches (the call does not carry K).
hipError_t launch_max_index(const int32_t* idx, int64_t n, int32_t* result, hipStream_t st);
// dst[dst_index[p] H + h] = src[p H + h]: a plan's clustered edge order back into the caller's (H words per edge).
hipError_t launch_scatter_heads(const float* src, const int32_t* dst_index, float* dst, int64_t nnz, int64_t H, hipStream_t st);

}  // namespace gespmm

#ifdef GESPMM_SDDMM_HEADS_KERNELS
#include "sddmm_edge.h"

namespace gespmm {

template <class OP, int V, int W, bool CSR>
__global__ __launch_bounds__(kThreads) void sddmm_heads_kernel(const int32_t* __restrict__ rows, const int32_t* __restrict__ colind,
                                                                const typename OP::elem* __restrict__ D1,
                                                                const typename OP::elem* __restrict__ D2, float* __restrict__ out, int M,
                                                                int nnz, int H, int F, int epw, uint32_t magic) {
    constexpr int G = 64 / W;
    constexpr int EPW = 256;  // most edges a wavefront owns (epw <= EPW): one row search per epw edges, ids of epw edges in LDS
    constexpr int UE = 4;     // pairs per lane group per step
    constexpr int IT = OP::template it<V>();  // vectors per lane that cover a head slice under resolve_sddmm's width rule
    using E = typename OP::elem;
    using T = typename OP::template vec<V>;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / W;
    const int l = lane % W;

    // ---- the wavefront's edges [e_lo, e_hi), its pairs [e_lo H, e_hi H), and where the (row, column) ids of an edge come from.
    // CSR form: as in sddmm_kernel — ONE wavefront-wide search for the row of the first edge, the epw + 2 row pointers from there in
    // LDS, every lane resolves one edge (the whole-array search when more than epw empty rows fall into the window). The ids are then
    // read H times. COO form: the caller's arrays at q / H.
    __shared__ int s_rp[CSR ? kWaves : 1][CSR ? EPW + 2 : 1];
    __shared__ int s_row[CSR ? kWaves : 1][CSR ? EPW : 1];
    __shared__ int s_col[CSR ? kWaves : 1][CSR ? EPW : 1];
    const int e_lo = (blockIdx.x * kWaves + wave) * epw;
    if (e_lo >= nnz) return;  // whole wavefront
    const int e_hi = (e_lo + epw < nnz) ? e_lo + epw : nnz;
    if constexpr (CSR) {
        const int r0 = row_of_edge_wave(rows, M, e_lo, lane);
        for (int i = lane; i < epw + 2; i += 64) s_rp[wave][i] = (r0 + i <= M) ? rows[r0 + i] : 0x7fffffff;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int e = e_lo + lane; e < e_hi; e += 64) {
            int lo = 0;
            if (s_rp[wave][1] <= e) {
                // largest i in [0, epw + 1] with s_rp[i] <= e   (s_rp[0] = rowptr[r0] <= e_lo <= e)
                int hi = epw + 1;
                if (s_rp[wave][hi] <= e) {  // more than epw empty rows in the window: search the whole array
                    lo = row_of_edge(rows, M, e) - r0;
                    hi = lo + 1;
                }
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (s_rp[wave][mid] <= e) lo = mid;
                    else hi = mid;
                }
            }
            s_row[wave][e - e_lo] = r0 + lo;
            s_col[wave][e - e_lo] = colind[e];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    const int q_lo = e_lo * H, q_hi = e_hi * H;  // (nnz H <= kSddmmMaxNnz: 32-bit pair arithmetic)
    const size_t ld = (size_t)H * (size_t)F;     // floats between two rows of D1 / D2
    // Pair q of this wavefront -> its two head slices. A pair past the wavefront's end takes the last valid pair (re-read, dropped at the
    // store). The edge is t / H on the wavefront-relative pair t < epw H: a host-made multiply-shift where that is exact, else the division.
    auto slices = [&](int q, const E*& p1, const E*& p2) {
        const unsigned t = (unsigned)((q < q_hi ? q : q_hi - 1) - q_lo);
        const unsigned er = magic ? __umulhi(t, magic) : t / (unsigned)H;
        const unsigned h = t - er * (unsigned)H;
        const int row = CSR ? s_row[wave][er] : rows[e_lo + (int)er];
        const int col = CSR ? s_col[wave][er] : colind[e_lo + (int)er];
        p1 = D1 + (size_t)row * ld + (size_t)h * (size_t)F;
        p2 = D2 + (size_t)col * ld + (size_t)h * (size_t)F;
    };

    for (int rb = 0; rb < q_hi - q_lo; rb += G * UE) {
        const int qbase = q_lo + rb + g * UE;
        float part[UE];
        if (F <= W * V) {
            // one vector per lane and slice: all 2 * UE vectors of the group's UE pairs are requested before any is used
            T x[UE], y[UE];
            const int j = l * V;
            const int jj = j < F ? j : 0;
#pragma unroll
            for (int u = 0; u < UE; ++u) {
                const E *p1, *p2;
                slices(qbase + u, p1, p2);
                x[u] = *reinterpret_cast<const T*>(p1 + jj);
                y[u] = *reinterpret_cast<const T*>(p2 + jj);
            }
#pragma unroll
            for (int u = 0; u < UE; ++u) {
                if (j >= F) {  // (a lane past the slice contributes fmaf(0, 0, 0), as in sddmm_kernel)
                    x[u] = T{};
                    y[u] = T{};
                }
                part[u] = OP::template dot<V>(x[u], y[u], 0.0f);
            }
        } else if (F <= W * V * IT) {
            // a lane walks up to IT vectors of each slice: two pairs at a time, all 4 * IT vectors requested before the first FMA
#pragma unroll
            for (int u0 = 0; u0 < UE; u0 += 2) {
                T x[2][IT], y[2][IT];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const E *p1, *p2;
                    slices(qbase + u0 + u, p1, p2);
#pragma unroll
                    for (int it = 0; it < IT; ++it) {
                        const int j = l * V + it * W * V;
                        x[u][it] = *reinterpret_cast<const T*>(p1 + (j < F ? j : 0));
                        y[u][it] = *reinterpret_cast<const T*>(p2 + (j < F ? j : 0));
                    }
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    float acc = 0.0f;
#pragma unroll
                    for (int it = 0; it < IT; ++it) {
                        if (l * V + it * W * V < F)  // the FMAs of the plain loop, in its order
                            acc = OP::template dot<V>(x[u][it], y[u][it], acc);
                    }
                    part[u0 + u] = acc;
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < UE; ++u) {
                const E *p1, *p2;
                slices(qbase + u, p1, p2);
                part[u] = 0.0f;
                for (int j = l * V; j < F; j += W * V) {
                    const T x = *reinterpret_cast<const T*>(p1 + j);
                    const T y = *reinterpret_cast<const T*>(p2 + j);
                    part[u] = OP::template dot<V>(x, y, part[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < UE; ++u) {
#pragma unroll
            for (int m = W >> 1; m > 0; m >>= 1) part[u] += __shfl_xor(part[u], m, 64);
            if (l == 0 && qbase + u < q_hi) out[qbase + u] = part[u];
        }
    }
}

template <class OP, int V, bool CSR>
static hipError_t sddmm_heads_w(int W, const int32_t* rows, const int32_t* colind, const typename OP::elem* D1,
                                const typename OP::elem* D2, float* out, int M, int nnz, int H, int F, int epw, uint32_t magic,
                                hipStream_t st) {
    const int nblk = (int)(((int64_t)nnz + kWaves * epw - 1) / (kWaves * epw));
#define GESPMM_SDH(WW)                                                                                                         \
    case WW:                                                                                                                    \
        hipLaunchKernelGGL((sddmm_heads_kernel<OP, V, WW, CSR>), dim3(nblk), dim3(kThreads), 0, st, rows, colind, D1, D2, out, M, \
                           nnz, H, F, epw, magic);                                                                              \
        return hipGetLastError();
    switch (W) {
        GESPMM_SDH(4)
        GESPMM_SDH(8)
        GESPMM_SDH(16)
        GESPMM_SDH(32)
        GESPMM_SDH(64)
    }
#undef GESPMM_SDH
    return hipErrorInvalidValue;
}

// Launches what resolve_sddmm_heads answered (r.route == kSddmmHeadsKernel), for the operand type OP.
template <class OP>
static hipError_t launch_sddmm_heads_op(const int32_t* rows, const int32_t* colind, const typename OP::elem* D1,
                                        const typename OP::elem* D2, float* out, int64_t M, int64_t nnz, int64_t H, int64_t F,
                                        const SddmmHeadsLaunch& r, hipStream_t st) {
    if (nnz == 0) return hipSuccess;
    if (r.route != kSddmmHeadsKernel || r.epw < 1 || r.epw > 256 || H < 1 || F < 1 || nnz * H > kSddmmMaxNnz) return hipErrorInvalidValue;
    const int m = (int)M, z = (int)nnz, h = (int)H, f = (int)F;
    const bool csr = r.form == kSddmmCsrEdge;
    if constexpr (OP::kMaxV >= 8)
        if (r.V == 8)
            return csr ? sddmm_heads_w<OP, 8, true>(r.W, rows, colind, D1, D2, out, m, z, h, f, r.epw, r.magic, st)
                       : sddmm_heads_w<OP, 8, false>(r.W, rows, colind, D1, D2, out, m, z, h, f, r.epw, r.magic, st);
    if (r.V == 4)
        return csr ? sddmm_heads_w<OP, 4, true>(r.W, rows, colind, D1, D2, out, m, z, h, f, r.epw, r.magic, st)
                   : sddmm_heads_w<OP, 4, false>(r.W, rows, colind, D1, D2, out, m, z, h, f, r.epw, r.magic, st);
    if (r.V == 2)
        return csr ? sddmm_heads_w<OP, 2, true>(r.W, rows, colind, D1, D2, out, m, z, h, f, r.epw, r.magic, st)
                   : sddmm_heads_w<OP, 2, false>(r.W, rows, colind, D1, D2, out, m, z, h, f, r.epw, r.magic, st);
    if (r.V == 1)
        return csr ? sddmm_heads_w<OP, 1, true>(r.W, rows, colind, D1, D2, out, m, z, h, f, r.epw, r.magic, st)
                   : sddmm_heads_w<OP, 1, false>(r.W, rows, colind, D1, D2, out, m, z, h, f, r.epw, r.magic, st);
    return hipErrorInvalidValue;
}

}  // namespace gespmm
#endif  // GESPMM_SDDMM_HEADS_KERNELS
