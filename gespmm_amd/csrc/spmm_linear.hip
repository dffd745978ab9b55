// spmm_linear.hip — fused aggregate-and-linear on fp16 / bf16 features (spmm_linear.h): one 256-thread workgroup per 64 consecutive
// rows, two phases around one barrier.
//
// Phase 1, aggregate into LDS. Wavefront w owns rows 16 w .. 16 w + 15 of the block and walks them G = 64 / W at a time, W lanes per
// row, a lane holding WPL 32-bit words (two elements each) of the row of H: W = 4 .. 64 with one word at K <= 128, W = 64 with two
// words (l and l + 64) beyond. A lane group loads max(W, 8) column indices (and weights) of its row with one coalesced load per lane
// and hands them round by lane index; gathers are issued eight at a time and consumed in CSR order, so each element is the ONE fp32
// chain of the 16-bit product (spmm_stream.h), multiplied once by row_scale and rounded once. The rounded row goes to an LDS tile
// [64][K_pad + 8] of 16-bit elements, K_pad = roundup(K, 16): columns K .. K_pad - 1 and rows past M are zero, and the 16 bytes of
// padding per row keep the 32 rows of a phase-2 read off one bank group. A hub row is walked by its one lane group.
//
// Phase 2, the matrix unit. v_mfma_f32_32x32x16_{f16,bf16}: lane l holds, of A, row l % 32 and the 8 consecutive k of half l / 32; of
// B, column l % 32 and the same 8 k; of the 32 x 32 result, column l % 32 and rows 8 (v / 4) + 4 (l / 32) + v % 4 in register v. A is
// a 16-byte LDS read of the tile; B is a 16-byte global load of W[n, k0 + 8 (l / 32) ..] — torch.nn.Linear's layout as it is, no
// transposed copy; W is at most 128 KB and stays in L2. Wavefront w owns the 32-column slabs w, w + 4 of the output, one after the
// other, and both 32-row halves of the block: a B fragment is loaded once per block and used for two row tiles (32 accumulators per
// lane). The root term X_root @ W_r^T is a second k loop into the same accumulators; its A fragments come straight from global
// memory (a row of X_root is contiguous: 16 bytes per lane), which keeps the workgroup at one LDS tile. Then bias (one fp32 add), one
// rounding, 2-byte stores of 32 consecutive columns per row; rows >= M and columns >= N_out are masked.
//
// No scratch, no atomics, no allocation: {fp16, bf16} x {valued, unweighted} x six lane geometries = 24 kernels. Compiled without
// packed fp32 arithmetic.

#include "spmm_linear.h"
#include "spmm_tile_mfma.h"

namespace gespmm {

template <int DT, bool VALUED, int W, int WPL>
__global__ __launch_bounds__(kThreads) void spmm_linear_kernel(const SpmmLinearArgs a) {
    static_assert(WPL == 1 || W == 64, "two words per lane only with a whole wavefront per row");
    extern __shared__ __attribute__((aligned(16))) unsigned char tile_raw[];
    constexpr int G = 64 / W;         // rows a wavefront walks at once
    constexpr int T = W > 8 ? W : 8;  // entries a lane group loads at once
    constexpr int E = T / W;          // ... per lane (2 at W = 4)
    constexpr int U = 8;              // gathers in flight per lane
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / W, l = lane % W;
    const int Kw = a.K >> 1;                   // words of a row of X / H
    const int Kpw = ((a.K + 15) & ~15) >> 1;   // ... of a padded tile row
    const int stride_w = Kpw + 4;              // ... and of the tile's row stride (16 bytes of padding)
    uint32_t* tile = reinterpret_cast<uint32_t*>(tile_raw);
    const int row0 = (int)blockIdx.x * kLinearBlockRows;

    // ------------------------------------------------------------------------- phase 1
    int wi[WPL];
    bool wok[WPL];
#pragma unroll
    for (int i = 0; i < WPL; ++i) {
        wi[i] = l + 64 * i;
        wok[i] = wi[i] < Kw;
    }
    for (int b = 0; b < 16; b += G) {
        const int tr = wave * 16 + b + g;  // tile row
        const int r = row0 + tr;
        int pos = 0, hb = 0;
        float rs = 1.0f;  // (x * 1.0f keeps every bit pattern the chain can produce)
        if (r < a.M) {
            pos = a.rowptr[r];
            hb = a.rowptr[r + 1];
            if (a.row_scale != nullptr) rs = a.row_scale[r];
        }
        float acc[2 * WPL];
#pragma unroll
        for (int i = 0; i < 2 * WPL; ++i) acc[i] = 0.0f;

        // Wave-uniform loops, per-lane predicates: every lane takes every step, so the lane-index exchange below always reads a live
        // lane. Slots past the row's end hold column 0 (a valid row of X: some group of the wavefront has an entry) and are not consumed.
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
                if (__builtin_amdgcn_ballot_w64(s < cnt) == 0) break;
                float v[U];
                float wd[U][WPL];
#pragma unroll
                for (int j = 0; j < U; ++j) {
                    const int e = (E == 1) ? 0 : j / W;  // (W = 4: one step of eight, entry j in slot j / 4 of lane j % 4)
                    const int src = (s + j) % W;
                    const int c = __shfl(pc[e], src, W);
                    if constexpr (VALUED) v[j] = __shfl(pv[e], src, W);
                    else v[j] = 1.0f;
                    const float* xrow = a.X + (uint32_t)c * (uint32_t)Kw;
#pragma unroll
                    for (int i = 0; i < WPL; ++i) wd[j][i] = xrow[wok[i] ? wi[i] : 0];
                }
#pragma unroll
                for (int j = 0; j < U; ++j)
                    if (s + j < cnt) accumulate_x16<DT, VALUED, WPL>(acc, v[j], wd[j]);
            }
            pos += T;
        }

        uint32_t* trow = tile + tr * stride_w;
#pragma unroll
        for (int i = 0; i < WPL; ++i)
            if (wok[i]) trow[wi[i]] = narrow_x16<DT>(fl32(__fmul_rn(acc[2 * i], rs))) | (narrow_x16<DT>(fl32(__fmul_rn(acc[2 * i + 1], rs))) << 16);
        for (int wz = Kw + l; wz < Kpw; wz += W) trow[wz] = 0u;
    }
    __syncthreads();

    // ------------------------------------------------------------------------- phase 2
    const int li = lane & 31, kh = lane >> 5;
    const int Kp = Kpw * 2;
    const int stride_b = stride_w * 4;
    const int nslab = (a.N_out + 31) >> 5;
    const uint16_t* Wn = static_cast<const uint16_t*>(a.W);
    const uint16_t* Wr = static_cast<const uint16_t*>(a.Wroot);
    const uint16_t* Xr = static_cast<const uint16_t*>(a.Xroot);
    uint16_t* out = static_cast<uint16_t*>(a.out);
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    for (int slab = wave; slab < nslab; slab += kWaves) {
        const int n = slab * 32 + li;
        const bool nok = n < a.N_out;
        floatx16 acc0, acc1;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            acc0[v] = 0.0f;
            acc1[v] = 0.0f;
        }
        for (int k0 = 0; k0 < Kp; k0 += 16) {
            const int k = k0 + 8 * kh;
            uint4 bf = zero;
            if (nok && k < a.K) bf = *reinterpret_cast<const uint4*>(Wn + n * a.K + k);
            const uint4 a0 = *reinterpret_cast<const uint4*>(tile_raw + li * stride_b + k * 2);
            const uint4 a1 = *reinterpret_cast<const uint4*>(tile_raw + (32 + li) * stride_b + k * 2);
            acc0 = mfma_32x32x16<DT>(a0, bf, acc0);
            acc1 = mfma_32x32x16<DT>(a1, bf, acc1);
        }
        if (Xr != nullptr) {
            const int r0 = row0 + li, r1 = r0 + 32;
            for (int k0 = 0; k0 < Kp; k0 += 16) {
                const int k = k0 + 8 * kh;
                uint4 bf = zero, a0 = zero, a1 = zero;
                if (k < a.K) {
                    if (nok) bf = *reinterpret_cast<const uint4*>(Wr + n * a.K + k);
                    if (r0 < a.M) a0 = *reinterpret_cast<const uint4*>(Xr + (uint32_t)r0 * (uint32_t)a.K + k);
                    if (r1 < a.M) a1 = *reinterpret_cast<const uint4*>(Xr + (uint32_t)r1 * (uint32_t)a.K + k);
                }
                acc0 = mfma_32x32x16<DT>(a0, bf, acc0);
                acc1 = mfma_32x32x16<DT>(a1, bf, acc1);
            }
        }
        const bool has_bias = a.bias != nullptr;
        const float bv = (has_bias && nok) ? a.bias[n] : 0.0f;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int r = row0 + 8 * (v / 4) + 4 * kh + (v % 4);
            float x0 = acc0[v], x1 = acc1[v];
            if (has_bias) {  // (NULL skips the add: x + 0.0f would turn -0.0 into +0.0)
                x0 = fl32(__fadd_rn(x0, bv));
                x1 = fl32(__fadd_rn(x1, bv));
            }
            if (nok && r < a.M) out[(uint32_t)r * (uint32_t)a.N_out + n] = (uint16_t)narrow_x16<DT>(x0);
            if (nok && r + 32 < a.M) out[(uint32_t)(r + 32) * (uint32_t)a.N_out + n] = (uint16_t)narrow_x16<DT>(x1);
        }
    }
}

template <int DT, bool VALUED, int W, int WPL>
static hipError_t launch_linear(const SpmmLinearArgs& a, hipStream_t st) {
    const int Kp = (a.K + 15) & ~15;
    const size_t lds = (size_t)kLinearBlockRows * (size_t)(2 * Kp + 16);
    const unsigned blocks = (unsigned)(((int64_t)a.M + kLinearBlockRows - 1) / kLinearBlockRows);
    hipLaunchKernelGGL((spmm_linear_kernel<DT, VALUED, W, WPL>), dim3(blocks), dim3(kThreads), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_spmm_linear_x16(const SpmmLinearArgs& a, int dtype, hipStream_t st) {
    if (!spmm_linear_served(a.M, 0, a.K, a.N_out, 0, 16)) return hipErrorInvalidValue;
    return dispatch_x16_valued(dtype, a.val != nullptr, [&](auto dt, auto valued) {
        return dispatch_lane_group<kLinearMaxK / 2>(a.K / 2, [&](auto w, auto wpl) {  // words per row
            return launch_linear<decltype(dt)::value, decltype(valued)::value, decltype(w)::value, decltype(wpl)::value>(a, st);
        });
    });
}

}  // namespace gespmm
