// spmm_relational_f32.hip — relational aggregate-and-linear on fp32 features (spmm_relational_f32.h): one 256-thread workgroup per 64
// consecutive output rows, a loop over the R relations of a stacked CSR, one fp32 LDS tile and one set of matrix-unit accumulators.
// Its own body: the 16-bit kernels (spmm_relational.hip) pack two elements per word and feed v_mfma_f32_32x32x16; here a lane holds a
// float4 of a row, the tile is fp32 and the matrix instruction is v_mfma_f32_32x32x2_f32, whose fragment is ONE k per lane.
//
// Per relation r, two phases between two barriers — unless the block has no entry of r: rowptr[r M + row0] == rowptr[r M + rend] is
// the same for every thread of the workgroup, and such a (block, relation) pair takes no tile write, no barrier and no MFMA.
//
// Phase 1, aggregate rows r M + row0 .. of the stacked CSR into the LDS tile [64][K_pad + 4] floats, K_pad = roundup(K, 8). W = 4 .. 64
// lanes cover a row, one float4 each (the smallest power of two >= K / 4, lanes past K / 4 masked); wavefront w owns tile rows
// 16 w .. 16 w + 15 and walks 64 / W of them at a time. A lane group loads max(W, 8) column indices (and weights) with one coalesced
// load per lane and hands them round by lane index; that exchange is unconditional. The 16-byte gather of a row of X is issued only for
// the slots s + j < cnt of the lane group's own row, eight in flight per lane, and steps past the wavefront's largest remaining count
// are not taken. Each element is the ONE fp32 chain of the fp32 product (fmaf(val, x, acc), or acc + x), multiplied once by row_scale.
//
// Phase 2, the matrix unit. v_mfma_f32_32x32x2_f32 wants from lane (li, kh) = (l % 32, l / 32) the element A[li][k] and B[k][li] of ONE
// k, that of half kh. A k step of 8: the lane reads one float4 of the tile, tile[row][k0 + 4 kh .. + 3] (one 16-byte LDS read per row
// half), and one float4 of W[r][n][k0 + 4 kh ..] (16 contiguous bytes of [N_out, K]: no transposed copy), and issues four MFMAs; the
// j-th takes component j of both, i.e. multiplies the pair k in {k0 + j, k0 + 4 + j}. A wavefront holds the accumulators of ALL its
// output across the relation loop: NS = 1 slab (w) when N_out <= 128, NS = 2 slabs (w, w + 4) beyond, times both 32-row halves — 32 or
// 64 accumulators per lane. After the loop the root term X_root @ W_root^T is one more k loop with A fragments from global memory, then
// bias (one fp32 add) and masked 4-byte stores.
//
// No scratch, no atomics, no allocation: {valued, unweighted} x five lane geometries x NS = 20 kernels. The tile is static LDS, sized
// by the geometry's K_pad class (<= 64, <= 128, <= 256). Compiled without packed fp32 arithmetic.

#include "spmm_relational_f32.h"
#include "spmm_tile_mfma.h"

namespace gespmm {

constexpr int rel_f32_kpad_class(int W) { return W <= 16 ? 64 : (W == 32 ? 128 : 256); }

// four MFMAs of one k step: component j of a and b is the lane's ONE k of the j-th instruction
__device__ __forceinline__ floatx16 rel_f32_mfma4(floatx4 a, floatx4 b, floatx16 c) {
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], b[2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], b[3], c, 0, 0, 0);
    return c;
}

template <bool VALUED, int W, int NS>
__global__ __launch_bounds__(kThreads) void spmm_relational_f32_kernel(const SpmmRelationalF32Args a) {
    constexpr int KPC = rel_f32_kpad_class(W);
    __shared__ __attribute__((aligned(16))) float tile[kLinearBlockRows * (KPC + 4)];
    constexpr int G = 64 / W;         // rows a wavefront walks at once
    constexpr int T = W > 8 ? W : 8;  // entries a lane group loads at once
    constexpr int E = T / W;          // ... per lane (2 at W = 4)
    constexpr int U = 8;              // gather slots per step
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / W, l = lane % W;
    const int Kp = (a.K + 7) & ~7;  // columns of a padded tile row
    const int stride = Kp + 4;      // ... and the tile's row stride in floats (16 bytes of padding)
    const int row0 = (int)blockIdx.x * kLinearBlockRows;
    const int rend = row0 + kLinearBlockRows < a.M ? row0 + kLinearBlockRows : a.M;
    const bool wok = 4 * l < a.K;        // the lane holds a float4 of the row
    const int xoff = wok ? 4 * l : 0;    // (a masked lane reads the row's first vector and drops it)
    const floatx4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};

    // columns K .. K_pad - 1 of the tile (one float4, when K % 8 == 4) are zero for every relation: written once, by the first masked lane
    if (4 * l == a.K && a.K < Kp)
        for (int b = 0; b < 16; b += G) *reinterpret_cast<floatx4*>(tile + (wave * 16 + b + g) * stride + a.K) = zero4;

    const int li = lane & 31, kh = lane >> 5;
    const int nslab = (a.N_out + 31) >> 5;
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
            float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};

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
                    floatx4 xv[U];
#pragma unroll
                    for (int j = 0; j < U; ++j) {
                        const int e = (E == 1) ? 0 : j / W;  // (W = 4: one step of eight, entry j in slot j / 4 of lane j % 4)
                        const int src = (s + j) % W;
                        const int c = __shfl(pc[e], src, W);
                        if constexpr (VALUED) v[j] = __shfl(pv[e], src, W);
                        else v[j] = 1.0f;
                        xv[j] = zero4;
                        if (s + j < cnt) xv[j] = *reinterpret_cast<const floatx4*>(a.X + (uint32_t)c * (uint32_t)a.K + xoff);  // (Kn K <= 2^31 - 4097)
                    }
#pragma unroll
                    for (int j = 0; j < U; ++j)
                        if (s + j < cnt) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) sum[i] = combine<kReduceSum, VALUED>(sum[i], v[j], xv[j][i]);
                        }
                }
                pos += T;
            }

            if (wok) {
                floatx4 h;
#pragma unroll
                for (int i = 0; i < 4; ++i) h[i] = __fmul_rn(sum[i], rs);
                *reinterpret_cast<floatx4*>(tile + tr * stride + 4 * l) = h;  // (rows >= M: zeros)
            }
        }
        __syncthreads();

        // --------------------------------------------------------------------- phase 2
        const float* Wn = a.W + (uint32_t)rel * (uint32_t)(a.N_out * a.K);  // (R N_out K <= 2^31 - 4097)
        if (sok[0]) {
            for (int k0 = 0; k0 < Kp; k0 += 8) {
                const int k = k0 + 4 * kh;
                const floatx4 a0 = *reinterpret_cast<const floatx4*>(tile + li * stride + k);
                const floatx4 a1 = *reinterpret_cast<const floatx4*>(tile + (32 + li) * stride + k);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if (!sok[s]) continue;
                    floatx4 bf = zero4;
                    if (nok[s] && k < a.K) bf = *reinterpret_cast<const floatx4*>(Wn + n[s] * a.K + k);
                    acc[s][0] = rel_f32_mfma4(a0, bf, acc[s][0]);
                    acc[s][1] = rel_f32_mfma4(a1, bf, acc[s][1]);
                }
            }
        }
        __syncthreads();  // the next relation overwrites the tile
    }

    // ----------------------------------------------------------------------------- root term, bias, store
    if (a.Xroot != nullptr && sok[0]) {
        const int r0 = row0 + li, r1 = r0 + 32;
        for (int k0 = 0; k0 < Kp; k0 += 8) {
            const int k = k0 + 4 * kh;
            floatx4 a0 = zero4, a1 = zero4;
            if (k < a.K) {
                if (r0 < a.M) a0 = *reinterpret_cast<const floatx4*>(a.Xroot + (uint32_t)r0 * (uint32_t)a.K + k);
                if (r1 < a.M) a1 = *reinterpret_cast<const floatx4*>(a.Xroot + (uint32_t)r1 * (uint32_t)a.K + k);
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                if (!sok[s]) continue;
                floatx4 bf = zero4;
                if (nok[s] && k < a.K) bf = *reinterpret_cast<const floatx4*>(a.Wroot + n[s] * a.K + k);
                acc[s][0] = rel_f32_mfma4(a0, bf, acc[s][0]);
                acc[s][1] = rel_f32_mfma4(a1, bf, acc[s][1]);
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
                x0 = __fadd_rn(x0, bv);
                x1 = __fadd_rn(x1, bv);
            }
            if (nok[s] && r < a.M) a.out[(uint32_t)r * (uint32_t)a.N_out + n[s]] = x0;
            if (nok[s] && r + 32 < a.M) a.out[(uint32_t)(r + 32) * (uint32_t)a.N_out + n[s]] = x1;
        }
    }
}

template <bool VALUED, int W>
static hipError_t launch_relational_f32(const SpmmRelationalF32Args& a, hipStream_t st) {
    const unsigned blocks = (unsigned)(((int64_t)a.M + kLinearBlockRows - 1) / kLinearBlockRows);
    if (a.N_out > 128) hipLaunchKernelGGL((spmm_relational_f32_kernel<VALUED, W, 2>), dim3(blocks), dim3(kThreads), 0, st, a);
    else hipLaunchKernelGGL((spmm_relational_f32_kernel<VALUED, W, 1>), dim3(blocks), dim3(kThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_spmm_relational_f32(const SpmmRelationalF32Args& a, hipStream_t st) {
    if (!spmm_relational_f32_served(a.R, a.M, 0, a.K, a.N_out, 0, 16)) return hipErrorInvalidValue;
    return dispatch_lane_group<kRelF32MaxK / 4>(a.K / 4, [&](auto w, auto) {  // float4 vectors per row
        return a.val != nullptr ? launch_relational_f32<true, decltype(w)::value>(a, st) : launch_relational_f32<false, decltype(w)::value>(a, st);
    });
}

}  // namespace gespmm
