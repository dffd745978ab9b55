// spmm_relational_wgrad.hip — fused relational weight gradient on fp16 / bf16 features (spmm_relational_wgrad.h):
// grad_W[r] = grad_out^T @ H_r with no H_r in memory. The reduction runs over the graph's rows, so the work split is not
// spmm_relational.hip's: a 256-thread workgroup owns (K-slab s, relation r, row chunk c) — blockIdx.x = (c R + r) slabs + s, one
// dimension because R is not bounded by a grid's y — walks the 64-row blocks of its chunk and keeps the [N_out, 64] partial of (r, s)
// in matrix-unit accumulators across the whole walk.
//
// A K-slab is 64 columns of X (the last one K - 64 s): a workgroup gathers only its slab's words of a row of X, so no gather is repeated
// across slabs. A (block, relation) pair with rowptr[r M + row0] == rowptr[r M + rend] — the same for every thread of the workgroup —
// takes no grad_out load, no barrier and no MFMA.
//
// Per block, phase 1: the rows r M + row0 .. are aggregated with spmm_relational.hip's walk (lane groups of W = 4 .. 32 lanes, one word
// per lane, the unconditional exchange by lane index, gathers only for the live slots of the group's own row, ONE fp32 chain, one
// multiply by row_scale, one rounding: the 16-bit product's bits) and written TRANSPOSED, HT[k][i] with a row stride of 64 + 8
// elements; the block's grad_out tile is staged transposed too, GT[n][i], from coalesced global loads of 16 / 8 / 4 / 2 bytes (the
// widest N_out allows), rows >= M as zeros. Phase 2, after one barrier: four reduction steps of 16 rows with
// v_mfma_f32_32x32x16_{f16,bf16}; the A fragment (row n = l % 32 of GT, eight consecutive i of half l / 32) and the B fragment (row
// k = l % 32 of HT, the same i) are one 16-byte LDS read each. Wavefront w owns the 32-row slabs w (and w + 4 when N_out > 128) of
// grad_W[r] times both 32-column halves of the K-slab: 32 or 64 accumulators per lane. A barrier before the next block overwrites the
// tiles. Rows n >= N_out of GT and rows k >= the slab's width of HT are never written: an MFMA row / column of garbage reaches only
// the output row / column of the same index, which is not stored.
//
// After the walk the accumulators go to partials[c][r][n][k] (zeros where everything was skipped); wgrad_reduce_kernel adds the C
// partials in the order c = 0 .. C - 1 in fp32 and rounds once. No scratch, no atomics, no allocation: {fp16, bf16} x {valued,
// unweighted} x four lane geometries x NS = 32 kernels and two reductions. Compiled without packed fp32 arithmetic.

#include "spmm_relational_wgrad.h"
#include "spmm_tile_mfma.h"

namespace gespmm {

// The block's grad_out tile, rows row0 .. row0 + 63 of [M, N_out] (contiguous in memory: 64 N_out elements), into GT[n][i]: V elements
// per load (V divides N_out, so a load stays inside a row and is V * 2 bytes aligned), consecutive threads consecutive addresses.
template <int V>
__device__ __forceinline__ void wg_stage_grad_out(const uint16_t* go, uint16_t* GT, int row0, int M, int N_out) {
    const uint16_t* src = go + (uint32_t)row0 * (uint32_t)N_out;  // (M N_out <= 2^31 - 4097)
    const int nv = kLinearBlockRows * N_out / V;
    for (int f = threadIdx.x; f < nv; f += kThreads) {
        const int e = f * V;
        const int i = e / N_out, n = e - i * N_out;
        uint16_t x[V];
#pragma unroll
        for (int j = 0; j < V; ++j) x[j] = 0;
        if (row0 + i < M) {
            if constexpr (V == 8) {
                const uint4 q = *reinterpret_cast<const uint4*>(src + e);
                const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = (uint16_t)(w[j / 2] >> (16 * (j % 2)));
            } else if constexpr (V == 4) {
                const uint2 q = *reinterpret_cast<const uint2*>(src + e);
                const uint32_t w[2] = {q.x, q.y};
#pragma unroll
                for (int j = 0; j < 4; ++j) x[j] = (uint16_t)(w[j / 2] >> (16 * (j % 2)));
            } else if constexpr (V == 2) {
                const uint32_t q = *reinterpret_cast<const uint32_t*>(src + e);
                x[0] = (uint16_t)q;
                x[1] = (uint16_t)(q >> 16);
            } else {
                x[0] = src[e];
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) GT[(n + j) * kWgradStride + i] = x[j];
    }
}

template <int DT, bool VALUED, int W, int NS>
__global__ __launch_bounds__(kThreads) void spmm_relational_wgrad_kernel(const SpmmRelationalWgradArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wg_lds[];
    constexpr int G = 64 / W;         // rows a wavefront walks at once
    constexpr int T = W > 8 ? W : 8;  // entries a lane group loads at once
    constexpr int E = T / W;          // ... per lane (2 at W = 4)
    constexpr int U = 8;              // gather slots per step
    uint16_t* HT = reinterpret_cast<uint16_t*>(wg_lds);  // [64][64 + 8]
    uint16_t* GT = HT + kWgradSlab * kWgradStride;       // [N_out rounded up to 32][64 + 8]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / W, l = lane % W;
    const int li = lane & 31, kh = lane >> 5;

    const uint32_t slabs = (uint32_t)(a.K + kWgradSlab - 1) / kWgradSlab;
    const uint32_t bid = blockIdx.x;  // (c R + r) slabs + s
    const int slab = (int)(bid % slabs);
    const int rel = (int)((bid / slabs) % (uint32_t)a.R), chunk = (int)((bid / slabs) / (uint32_t)a.R);
    const int k0 = slab * kWgradSlab;
    const int SW = a.K - k0 < kWgradSlab ? a.K - k0 : kWgradSlab;  // columns of this slab: a multiple of 8
    const int Kw = a.K >> 1;                                      // words of a row of X
    const bool wok = l < (SW >> 1);                               // the lane has a word of the slab
    const float* Xs = a.X + (k0 >> 1);
    const int nblk = (int)(((int64_t)a.M + kLinearBlockRows - 1) / kLinearBlockRows);  // (spmm_relational_wgrad_blocks)
    const int blk_lo = (int)((int64_t)chunk * nblk / a.C), blk_hi = (int)((int64_t)(chunk + 1) * nblk / a.C);
    const int base = rel * a.M;  // (R M <= 2^31 - 4097)
    const int gvec = a.N_out % 8 == 0 ? 8 : a.N_out % 4 == 0 ? 4 : a.N_out % 2 == 0 ? 2 : 1;
    const uint16_t* go = static_cast<const uint16_t*>(a.grad_out);

    const int nslab = (a.N_out + 31) >> 5;
    const bool two = SW > 32;  // the slab has a second 32-column half (workgroup-uniform)
    bool sok[NS];              // the wavefront has this slab of grad_W[r] at all (wave-uniform)
    floatx16 acc[NS][2];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        sok[s] = wave + kWaves * s < nslab;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            acc[s][0][v] = 0.0f;
            acc[s][1][v] = 0.0f;
        }
    }

    for (int blk = blk_lo; blk < blk_hi; ++blk) {
        const int row0 = blk * kLinearBlockRows;
        const int rend = row0 + kLinearBlockRows < a.M ? row0 + kLinearBlockRows : a.M;
        if (a.rowptr[base + row0] == a.rowptr[base + rend]) continue;  // workgroup-uniform: no entry of this relation in the block

        // --------------------------------------------------------------------- phase 1
        for (int b = 0; b < 16; b += G) {
            const int tr = wave * 16 + b + g;  // tile row i
            const int r = row0 + tr;
            int pos = 0, hb = 0;
            float rs = 1.0f;  // (x * 1.0f keeps every bit pattern the chain can produce)
            if (r < a.M) {
                pos = a.rowptr[base + r];
                hb = a.rowptr[base + r + 1];
                if (a.row_scale != nullptr) rs = a.row_scale[base + r];
            }
            float sum[2] = {0.0f, 0.0f};

            // Wave-uniform loops, per-lane predicates: every lane takes every step, so the lane-index exchange always reads a live lane.
            while (__builtin_amdgcn_ballot_w64(pos < hb) != 0) {
                int pc[E];
                float pv[E];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int p = pos + e * W + l;
                    pc[e] = 0;
                    pv[e] = 0.0f;
                    if (p < hb) {
                        pc[e] = load_csr(a.colind + p);
                        if constexpr (VALUED) pv[e] = load_csr(a.val + p);
                    }
                }
                const int cnt = hb - pos;  // entries of this group's row still to consume (<= 0: none)
#pragma unroll 1
                for (int s = 0; s < T; s += U) {
                    if (__builtin_amdgcn_ballot_w64(s < cnt) == 0) break;  // past the wavefront's largest remaining count
                    float v[U];
                    float wd[U][1];
#pragma unroll
                    for (int j = 0; j < U; ++j) {
                        const int e = (E == 1) ? 0 : j / W;  // (W = 4: one step of eight, entry j in slot j / 4 of lane j % 4)
                        const int src = (s + j) % W;
                        const int c = __shfl(pc[e], src, W);
                        if constexpr (VALUED) v[j] = __shfl(pv[e], src, W);
                        else v[j] = 1.0f;
                        wd[j][0] = 0.0f;
                        if (s + j < cnt) wd[j][0] = Xs[(uint32_t)c * (uint32_t)Kw + (wok ? l : 0)];  // (Kn K <= 2^31 - 4097)
                    }
#pragma unroll
                    for (int j = 0; j < U; ++j)
                        if (s + j < cnt) accumulate_x16<DT, VALUED, 1>(sum, v[j], wd[j]);
                }
                pos += T;
            }

            if (wok) {  // rows >= M of the block are written too, as zeros: the reduction runs over all 64
                HT[(2 * l) * kWgradStride + tr] = (uint16_t)narrow_x16<DT>(fl32(__fmul_rn(sum[0], rs)));
                HT[(2 * l + 1) * kWgradStride + tr] = (uint16_t)narrow_x16<DT>(fl32(__fmul_rn(sum[1], rs)));
            }
        }
        if (gvec == 8) wg_stage_grad_out<8>(go, GT, row0, a.M, a.N_out);
        else if (gvec == 4) wg_stage_grad_out<4>(go, GT, row0, a.M, a.N_out);
        else if (gvec == 2) wg_stage_grad_out<2>(go, GT, row0, a.M, a.N_out);
        else wg_stage_grad_out<1>(go, GT, row0, a.M, a.N_out);
        __syncthreads();

        // --------------------------------------------------------------------- phase 2
        if (sok[0]) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i0 = 16 * q + 8 * kh;
                const uint4 b0 = *reinterpret_cast<const uint4*>(HT + li * kWgradStride + i0);
                uint4 b1 = make_uint4(0u, 0u, 0u, 0u);
                if (two) b1 = *reinterpret_cast<const uint4*>(HT + (32 + li) * kWgradStride + i0);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if (!sok[s]) continue;
                    const uint4 af = *reinterpret_cast<const uint4*>(GT + ((wave + kWaves * s) * 32 + li) * kWgradStride + i0);
                    acc[s][0] = mfma_32x32x16<DT>(af, b0, acc[s][0]);
                    if (two) acc[s][1] = mfma_32x32x16<DT>(af, b1, acc[s][1]);
                }
            }
        }
        __syncthreads();  // the next block overwrites the tiles
    }

    // ----------------------------------------------------------------------------- the partial of (chunk, rel, slab)
    float* part = a.partials + ((uint32_t)chunk * (uint32_t)a.R + (uint32_t)rel) * (uint32_t)(a.N_out * a.K);  // (C R N_out K <= 2^31 - 4097)
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (!sok[s]) continue;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int n = (wave + kWaves * s) * 32 + 8 * (v / 4) + 4 * kh + (v % 4);
            if (n >= a.N_out) continue;
            if (li < SW) part[n * a.K + k0 + li] = acc[s][0][v];
            if (32 + li < SW) part[n * a.K + k0 + 32 + li] = acc[s][1][v];
        }
    }
}

// grad_W = narrow(partials[0] + partials[1] + .. + partials[C - 1]): one fp32 chain per element in that order, one rounding. A thread
// takes four consecutive elements (R N_out K is a multiple of 8).
template <int DT>
__global__ __launch_bounds__(kThreads) void wgrad_reduce_kernel(const float4* __restrict__ partials, uint2* __restrict__ out, uint32_t quads, int C) {
    const uint32_t idx = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (idx >= quads) return;
    float4 s = partials[idx];
    for (int c = 1; c < C; ++c) {
        const float4 p = partials[(uint32_t)c * quads + idx];
        s.x = __fadd_rn(s.x, p.x);
        s.y = __fadd_rn(s.y, p.y);
        s.z = __fadd_rn(s.z, p.z);
        s.w = __fadd_rn(s.w, p.w);
    }
    out[idx] = make_uint2(narrow_x16<DT>(fl32(s.x)) | (narrow_x16<DT>(fl32(s.y)) << 16),
                          narrow_x16<DT>(fl32(s.z)) | (narrow_x16<DT>(fl32(s.w)) << 16));
}

template <int DT, bool VALUED, int W>
static hipError_t launch_wgrad(const SpmmRelationalWgradArgs& a, hipStream_t st) {
    const int np = (a.N_out + 31) & ~31;
    const size_t lds = (size_t)(kWgradSlab + np) * kWgradStride * 2;  // 46080 bytes at N_out = 256
    const unsigned slabs = (unsigned)((a.K + kWgradSlab - 1) / kWgradSlab);
    const unsigned blocks = (unsigned)a.C * (unsigned)a.R * slabs;  // (C R N_out K <= 2^31 - 4097 and K / slabs >= 8: below 2^28)
    if (a.N_out > 128) hipLaunchKernelGGL((spmm_relational_wgrad_kernel<DT, VALUED, W, 2>), dim3(blocks), dim3(kThreads), lds, st, a);
    else hipLaunchKernelGGL((spmm_relational_wgrad_kernel<DT, VALUED, W, 1>), dim3(blocks), dim3(kThreads), lds, st, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    const uint32_t quads = (uint32_t)a.R * (uint32_t)(a.N_out * a.K) / 4;
    hipLaunchKernelGGL((wgrad_reduce_kernel<DT>), dim3((quads + kThreads - 1) / kThreads), dim3(kThreads), 0, st,
                       reinterpret_cast<const float4*>(a.partials), static_cast<uint2*>(a.grad_w), quads, a.C);
    return hipGetLastError();
}

hipError_t launch_spmm_relational_wgrad_x16(const SpmmRelationalWgradArgs& a, int dtype, hipStream_t st) {
    if (!spmm_relational_wgrad_served(a.R, a.M, 0, a.K, a.N_out, 0, a.C, 16)) return hipErrorInvalidValue;
    const int Sw = (a.K < kWgradSlab ? a.K : kWgradSlab) / 2;  // words of the widest slab
    return dispatch_x16_valued(dtype, a.val != nullptr, [&](auto dt, auto valued) {
        return dispatch_lane_group<kWgradSlab / 2>(Sw, [&](auto w, auto) {
            return launch_wgrad<decltype(dt)::value, decltype(valued)::value, decltype(w)::value>(a, st);
        });
    });
}

}  // namespace gespmm
