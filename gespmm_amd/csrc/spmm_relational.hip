// spmm_relational.hip — relational aggregate-and-linear on fp16 / bf16 features (spmm_relational.h): one 256-thread workgroup per 64
// consecutive output rows, a loop over the R relations of a stacked CSR, one LDS tile and one set of matrix-unit accumulators.
//
// Per relation r, two phases between two barriers — unless the block has no entry of r: rowptr[r M + row0] == rowptr[r M + rend] is
// the same for every thread of the workgroup, and such a (block, relation) pair takes no tile write, no barrier and no MFMA.
//
// Phase 1, aggregate rows r M + row0 .. of the stacked CSR into the LDS tile [64][K_pad + 8] (spmm_linear.hip's layout and lane
// geometries: W = 4 .. 64 lanes per row, one word per lane up to K = 128, two beyond). A lane group loads max(W, 8) column indices
// (and weights) with one coalesced load per lane and hands them round by lane index; that exchange is unconditional, every lane
// takes every step. The gather of a row of X is issued only for the slots s + j < cnt of the lane group's own row: rows of a
// relational graph hold a few entries each, so a row with one entry issues ONE gather where the unconditional walk issues eight. The
// chain consumes the same entries in the same order: each element is the ONE fp32 chain of the 16-bit product, multiplied once by
// row_scale and rounded once.
//
// Phase 2, the matrix unit: v_mfma_f32_32x32x16_{f16,bf16}, A fragments (16-byte LDS reads) from the tile, B fragments (16-byte global
// loads) straight from W[r] as [N_out, K]. A wavefront holds the accumulators of ALL its output across the relation loop: NS = 1
// slab (w) when N_out <= 128, NS = 2 slabs (w, w + 4) beyond, times both 32-row halves — 32 or 64 accumulators per lane. An A
// fragment is read once per k step and feeds every slab of the wavefront. After the loop the root term X_root @ W_root^T is one more k
// loop with A fragments from global memory, then bias (one fp32 add), one rounding, masked 2-byte stores.
//
// No scratch, no atomics, no allocation: {fp16, bf16} x {valued, unweighted} x six lane geometries x NS = 48 kernels. Compiled without
// packed fp32 arithmetic. GESPMM_RELATIONAL_DEAD_GATHERS (measurement only, never in the shipped library) issues every gather
// unconditionally, as spmm_linear.hip does.

#include "spmm_relational.h"
#include "spmm_tile_mfma.h"

namespace gespmm {

template <int DT, bool VALUED, int W, int WPL, int NS>
__global__ __launch_bounds__(kThreads) void spmm_relational_kernel(const SpmmRelationalArgs a) {
    static_assert(WPL == 1 || W == 64, "two words per lane only with a whole wavefront per row");
    extern __shared__ __attribute__((aligned(16))) unsigned char tile_raw[];
    constexpr int G = 64 / W;         // rows a wavefront walks at once
    constexpr int T = W > 8 ? W : 8;  // entries a lane group loads at once
    constexpr int E = T / W;          // ... per lane (2 at W = 4)
    constexpr int U = 8;              // gather slots per step
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / W, l = lane % W;
    const int Kw = a.K >> 1;                   // words of a row of X / H
    const int Kpw = ((a.K + 15) & ~15) >> 1;   // ... of a padded tile row
    const int stride_w = Kpw + 4;              // ... and of the tile's row stride (16 bytes of padding)
    uint32_t* tile = reinterpret_cast<uint32_t*>(tile_raw);
    const int row0 = (int)blockIdx.x * kLinearBlockRows;
    const int rend = row0 + kLinearBlockRows < a.M ? row0 + kLinearBlockRows : a.M;

    int wi[WPL];
    bool wok[WPL];
#pragma unroll
    for (int i = 0; i < WPL; ++i) {
        wi[i] = l + 64 * i;
        wok[i] = wi[i] < Kw;
    }
    // columns K .. K_pad - 1 of the tile are zero for every relation: written once, by the lanes that write the row
    for (int b = 0; b < 16; b += G) {
        uint32_t* trow = tile + (wave * 16 + b + g) * stride_w;
        for (int wz = Kw + l; wz < Kpw; wz += W) trow[wz] = 0u;
    }

    const int li = lane & 31, kh = lane >> 5;
    const int Kp = Kpw * 2;
    const int stride_b = stride_w * 4;
    const int nslab = (a.N_out + 31) >> 5;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    int n[NS];
    bool nok[NS], sok[NS];  // sok: the wavefront has this slab at all (wave-uniform)
    floatx16 acc[NS][2];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        n[s] = (wave + kWaves * s) * 32 + li;
        nok[s] = n[s] < a.N_out;
        sok[s] = wave + kWaves * s < nslab;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            acc[s][0][v] = 0.0f;
            acc[s][1][v] = 0.0f;
        }
    }

    for (int rel = 0; rel < a.R; ++rel) {
        const int base = rel * a.M;  // (R M <= 2^31 - 4097)
        if (a.rowptr[base + row0] == a.rowptr[base + rend]) continue;  // workgroup-uniform: no entry of this relation in the block

        // --------------------------------------------------------------------- phase 1
        for (int b = 0; b < 16; b += G) {
            const int tr = wave * 16 + b + g;  // tile row
            const int r = row0 + tr;
            int pos = 0, hb = 0;
            float rs = 1.0f;  // (x * 1.0f keeps every bit pattern the chain can produce)
            if (r < a.M) {
                pos = a.rowptr[base + r];
                hb = a.rowptr[base + r + 1];
                if (a.row_scale != nullptr) rs = a.row_scale[base + r];
            }
            float sum[2 * WPL];
#pragma unroll
            for (int i = 0; i < 2 * WPL; ++i) sum[i] = 0.0f;

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
                    float wd[U][WPL];
#pragma unroll
                    for (int j = 0; j < U; ++j) {
                        const int e = (E == 1) ? 0 : j / W;  // (W = 4: one step of eight, entry j in slot j / 4 of lane j % 4)
                        const int src = (s + j) % W;
                        const int c = __shfl(pc[e], src, W);
                        if constexpr (VALUED) v[j] = __shfl(pv[e], src, W);
                        else v[j] = 1.0f;
#ifdef GESPMM_RELATIONAL_DEAD_GATHERS
                        const bool live = true;  // (slots past the row's end hold column 0, a valid row of X)
#else
                        const bool live = s + j < cnt;
#endif
#pragma unroll
                        for (int i = 0; i < WPL; ++i) wd[j][i] = 0.0f;
                        if (live) {
                            const float* xrow = a.X + (uint32_t)c * (uint32_t)Kw;
#pragma unroll
                            for (int i = 0; i < WPL; ++i) wd[j][i] = xrow[wok[i] ? wi[i] : 0];
                        }
                    }
#pragma unroll
                    for (int j = 0; j < U; ++j)
                        if (s + j < cnt) accumulate_x16<DT, VALUED, WPL>(sum, v[j], wd[j]);
                }
                pos += T;
            }

            uint32_t* trow = tile + tr * stride_w;
#pragma unroll
            for (int i = 0; i < WPL; ++i)
                if (wok[i])
                    trow[wi[i]] = narrow_x16<DT>(fl32(__fmul_rn(sum[2 * i], rs))) | (narrow_x16<DT>(fl32(__fmul_rn(sum[2 * i + 1], rs))) << 16);
        }
        __syncthreads();

        // --------------------------------------------------------------------- phase 2
        const uint16_t* Wn = static_cast<const uint16_t*>(a.W) + (uint32_t)rel * (uint32_t)(a.N_out * a.K);  // (R N_out K <= 2^31 - 4097)
        if (sok[0]) {
            for (int k0 = 0; k0 < Kp; k0 += 16) {
                const int k = k0 + 8 * kh;
                const uint4 a0 = *reinterpret_cast<const uint4*>(tile_raw + li * stride_b + k * 2);
                const uint4 a1 = *reinterpret_cast<const uint4*>(tile_raw + (32 + li) * stride_b + k * 2);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if (!sok[s]) continue;
                    uint4 bf = zero;
                    if (nok[s] && k < a.K) bf = *reinterpret_cast<const uint4*>(Wn + n[s] * a.K + k);
                    acc[s][0] = mfma_32x32x16<DT>(a0, bf, acc[s][0]);
                    acc[s][1] = mfma_32x32x16<DT>(a1, bf, acc[s][1]);
                }
            }
        }
        __syncthreads();  // the next relation overwrites the tile
    }

    // ----------------------------------------------------------------------------- root term, bias, store
    const uint16_t* Wr = static_cast<const uint16_t*>(a.Wroot);
    const uint16_t* Xr = static_cast<const uint16_t*>(a.Xroot);
    uint16_t* out = static_cast<uint16_t*>(a.out);
    if (Xr != nullptr && sok[0]) {
        const int r0 = row0 + li, r1 = r0 + 32;
        for (int k0 = 0; k0 < Kp; k0 += 16) {
            const int k = k0 + 8 * kh;
            uint4 a0 = zero, a1 = zero;
            if (k < a.K) {
                if (r0 < a.M) a0 = *reinterpret_cast<const uint4*>(Xr + (uint32_t)r0 * (uint32_t)a.K + k);
                if (r1 < a.M) a1 = *reinterpret_cast<const uint4*>(Xr + (uint32_t)r1 * (uint32_t)a.K + k);
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                if (!sok[s]) continue;
                uint4 bf = zero;
                if (nok[s] && k < a.K) bf = *reinterpret_cast<const uint4*>(Wr + n[s] * a.K + k);
                acc[s][0] = mfma_32x32x16<DT>(a0, bf, acc[s][0]);
                acc[s][1] = mfma_32x32x16<DT>(a1, bf, acc[s][1]);
            }
        }
    }
    const bool has_bias = a.bias != nullptr;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (!sok[s]) continue;
        const float bv = (has_bias && nok[s]) ? a.bias[n[s]] : 0.0f;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int r = row0 + 8 * (v / 4) + 4 * kh + (v % 4);
            float x0 = acc[s][0][v], x1 = acc[s][1][v];
            if (has_bias) {  // (NULL skips the add: x + 0.0f would turn -0.0 into +0.0)
                x0 = fl32(__fadd_rn(x0, bv));
                x1 = fl32(__fadd_rn(x1, bv));
            }
            if (nok[s] && r < a.M) out[(uint32_t)r * (uint32_t)a.N_out + n[s]] = (uint16_t)narrow_x16<DT>(x0);
            if (nok[s] && r + 32 < a.M) out[(uint32_t)(r + 32) * (uint32_t)a.N_out + n[s]] = (uint16_t)narrow_x16<DT>(x1);
        }
    }
}

template <int DT, bool VALUED, int W, int WPL>
static hipError_t launch_relational(const SpmmRelationalArgs& a, hipStream_t st) {
    const int Kp = (a.K + 15) & ~15;
    const size_t lds = (size_t)kLinearBlockRows * (size_t)(2 * Kp + 16);
    const unsigned blocks = (unsigned)(((int64_t)a.M + kLinearBlockRows - 1) / kLinearBlockRows);
    if (a.N_out > 128) hipLaunchKernelGGL((spmm_relational_kernel<DT, VALUED, W, WPL, 2>), dim3(blocks), dim3(kThreads), lds, st, a);
    else hipLaunchKernelGGL((spmm_relational_kernel<DT, VALUED, W, WPL, 1>), dim3(blocks), dim3(kThreads), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_spmm_relational_x16(const SpmmRelationalArgs& a, int dtype, hipStream_t st) {
    if (!spmm_relational_served(a.R, a.M, 0, a.K, a.N_out, 0, 16)) return hipErrorInvalidValue;
    return dispatch_x16_valued(dtype, a.val != nullptr, [&](auto dt, auto valued) {
        return dispatch_lane_group<kLinearMaxK / 2>(a.K / 2, [&](auto w, auto wpl) {  // words per row
            return launch_relational<decltype(dt)::value, decltype(valued)::value, decltype(w)::value, decltype(wpl)::value>(a, st);
        });
    });
}

}  // namespace gespmm
