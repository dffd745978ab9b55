// gat_backward_group_kernel.h — the GROUP form of the fused GAT backward for el / er (gat_backward.h: contract and form rule) as a
// template on the element type of grad_out and feat. Included by gat_backward_group.hip (DT = 0: fp32 — the instruction streams are what
// they were when the body stood in that file) and by gat_backward_group_x16.hip (DT = kX16F16 / kX16Bf16). The lane form
// (gat_backward_kernel.h) lets ONE lane walk the whole dot g_p = <grad_out[r, h, :], feat[c, h, :]> of the entry it owns, so a
// load instruction of a wavefront touches 64 different lines for 16 bytes each. Here the dot is transposed inside the wavefront:
//
//   - segment geometry, regimes, entry ownership and every statement after g are the lane form's, restated statement for statement:
//     a (segment, head) pair per group of W_s lanes (a run-time, wave-uniform value here: 4 / 8 / 16, 64 in the hub branch), lane l owns
//     entries lo + l + t W_s and keeps w, g, f, dl of up to IT of them;
//   - the 64 lanes ALSO form 64 / W_d dot sub-groups of W_d contiguous lanes, (4, W_d) = resolve_sddmm's answer at width F (W_d the
//     smallest power of two in 4 .. 64 with 8 W_d >= F; a template parameter, independent of W_s). Per `it`, a sub-group takes W_d
//     steps; in step s it serves the entry owned by ITS lane s: the gathered row's offset and the fixed row's offset are broadcast from
//     that lane (a width-W_d shuffle — both, because with W_s < W_d the lanes of a sub-group belong to different pairs), lane q walks
//     words j = 4 q + i + 4 W_d t of both rows (t < 2) in one fmaf chain from +0, the xor butterfly W_d / 2 .. 1 follows, and lane s
//     keeps the sum. That is launch_sddmm_heads' chain at (4, W_d), in all of its forms: g has its bits on ANY operands.
//   - a load instruction now reads 64 / W_d rows as contiguous runs of 16 W_d bytes, and a wavefront issues as many of them per `it`
//     as the lane form (W_d steps of 2 F / (4 W_d) loads against 2 F / 4). The steps are independent: the loads of kU steps are
//     requested before the first is used. kU steps none of whose owners holds a live entry are skipped by a wave-uniform ballot.
//
// Safety rules (gat_backward.hip's): every load is of a valid word — a lane past its segment's end re-reads the segment's first entry,
// a lane past the head slice re-reads its first vector — and what it yields is dropped by a select; trip counts, the regime and the
// skip are wave-uniform; every shuffle is executed by all 64 lanes; only stores are predicated; a wavefront past S returns whole. No
// atomics, no LDS, no workspace. Word positions are 32-bit (M H F, K H F <= kSddmmMaxNnz), byte offsets are formed by pointer arithmetic.
//
// The fixed row is NOT kept in registers (it could be where W_d <= W_s): it is re-read per step through the L1, as in the lane form.
//
// 16-bit elements (DT != 0): lane q still walks ELEMENTS j = 4 q + i + 4 W_d t — one 8-byte load of four elements per vector, kept packed
// in two registers (half the fp32 form's) and widened exactly at the fmaf — so W_d, the lane positions and the butterfly are those of
// the fp32 form at width F, and g has its bits on the widened operands. A wavefront's load reads 64 / W_d rows as runs of 8 W_d bytes.
#pragma once

#include <math.h>

#include "edge_dropout.h"
#include "edge_softmax.h"
#include "gat_aggregate.h"
#include "gat_backward.h"
#include "spmm_device.h"
#include "spmm_kernels.h"

#ifndef GESPMM_GB_GROUP_U
#define GESPMM_GB_GROUP_U 4  // steps whose loads are in flight together (measured against 2: DESIGN 3.18)
#endif

namespace gespmm {
namespace {

constexpr int IT = kEdgeSoftmaxIT;  // entries a lane keeps in registers
constexpr int kU = GESPMM_GB_GROUP_U;

struct DropWords {  // (gat_backward.hip's)
    uint32_t s0, s1, threshold;
    float scale;
};

#define GESPMM_GBG_PTRS                                                                                                               \
    const int32_t *__restrict__ ind, const float *__restrict__ el, const float *__restrict__ er, const float2 *__restrict__ stats,    \
        const float *__restrict__ delta, const gb_elem_t<DT> *__restrict__ fixed, const gb_elem_t<DT> *__restrict__ gathered
#define GESPMM_GBG_ARGS ind, el, er, stats, delta, fixed, gathered

// group_sum / wave_max_degree of edge_softmax.h at a wave-uniform run-time W: the same statements behind a uniform switch.
__device__ __forceinline__ float group_sum_w(float v, int W) {
    switch (W) {
        case 4: return group_sum<4>(v);
        case 8: return group_sum<8>(v);
        case 16: return group_sum<16>(v);
    }
    return group_sum<64>(v);
}

__device__ __forceinline__ int wave_max_degree_w(int d, int W) {
    switch (W) {
        case 4: return wave_max_degree<4>(d);
        case 8: return wave_max_degree<8>(d);
        case 16: return wave_max_degree<16>(d);
    }
    return wave_max_degree<64>(d);
}

// Four consecutive elements of a row as a lane holds them until their fmaf: a float4, or two 32-bit words of two 16-bit elements each.
template <int DT>
struct GroupVec {
    using type = uint2;
};
template <>
struct GroupVec<0> {
    using type = float4;
};

__device__ __forceinline__ float chain4(const float4 a, const float4 b, float acc) {
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    return fmaf(a.w, b.w, acc);
}

// ... on packed 16-bit elements: each widened, exactly, at its fmaf — the same chain on the same values.
template <int DT>
__device__ __forceinline__ float chain4(const uint2 a, const uint2 b, float acc) {
    float a0, a1, a2, a3, b0, b1, b2, b3;
    widen_x16<DT>(__uint_as_float(a.x), a0, a1);
    widen_x16<DT>(__uint_as_float(a.y), a2, a3);
    widen_x16<DT>(__uint_as_float(b.x), b0, b1);
    widen_x16<DT>(__uint_as_float(b.y), b2, b3);
    acc = fmaf(a0, b0, acc);
    acc = fmaf(a1, b1, acc);
    acc = fmaf(a2, b2, acc);
    return fmaf(a3, b3, acc);
}

template <int DT>
__device__ __forceinline__ float chain_elems(const typename GroupVec<DT>::type a, const typename GroupVec<DT>::type b, float acc) {
    if constexpr (DT == 0) return chain4(a, b, acc);
    else return chain4<DT>(a, b, acc);
}

// The dots of one `it` for all 64 lanes: lane's own entry has the fixed row at word fo and the gathered row at word go (both valid
// for every lane), `live` says whether the lane owns an entry of its segment. -> the dot of the lane's own entry (0 where a step was
// skipped: no live owner). q: the lane's position in its dot sub-group. two: F > 4 W_d (wave-uniform): a second vector per lane.
template <int DT, int WD>
__device__ __forceinline__ float group_dots(const gb_elem_t<DT>* __restrict__ fixed, const gb_elem_t<DT>* __restrict__ gathered, int fo, int go, bool live,
                                            int F, int q, bool two) {
    constexpr uint64_t kEvery = ~0ull / ((WD == 64) ? ~0ull : ((1ull << WD) - 1));  // bit 0 of every sub-group
    constexpr uint64_t kChunk = kEvery * ((1ull << kU) - 1);                        // bits 0 .. kU - 1 of every sub-group
    static_assert(kU <= 4 && WD % kU == 0, "a chunk of steps stays inside a sub-group");
    using vec_t = typename GroupVec<DT>::type;
    const uint64_t lm = __ballot(live);
    const int j0 = 4 * q, j1 = 4 * q + 4 * WD;
    const bool in0 = j0 < F, in1 = two && j1 < F;
    const int c0 = in0 ? j0 : 0, c1 = in1 ? j1 : 0;
    float mine = 0.0f;
    for (int s0 = 0; s0 < WD; s0 += kU) {
        if (((lm >> s0) & kChunk) == 0) continue;  // wave-uniform: lm is a ballot
        vec_t a[kU][2], b[kU][2];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const gb_elem_t<DT>* __restrict__ pf = fixed + __shfl(fo, s0 + u, WD);
            const gb_elem_t<DT>* __restrict__ pg = gathered + __shfl(go, s0 + u, WD);
            a[u][0] = *reinterpret_cast<const vec_t*>(pf + c0);
            b[u][0] = *reinterpret_cast<const vec_t*>(pg + c0);
            if (two) {  // wave-uniform
                a[u][1] = *reinterpret_cast<const vec_t*>(pf + c1);
                b[u][1] = *reinterpret_cast<const vec_t*>(pg + c1);
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            float acc = 0.0f;
            const float x0 = chain_elems<DT>(a[u][0], b[u][0], acc);
            acc = in0 ? x0 : acc;  // (a lane past the slice: +0, what the SDDMM's fmaf(0, 0, 0) gives)
            if (two) {
                const float x1 = chain_elems<DT>(a[u][1], b[u][1], acc);
                acc = in1 ? x1 : acc;
            }
#pragma unroll
            for (int m = WD >> 1; m > 0; m >>= 1) acc += __shfl_xor(acc, m, 64);
            mine = (q == s0 + u) ? acc : mine;
        }
    }
    return mine;
}

// One (segment, head) pair per group of W lanes -> (delta, sum of gs): gat_backward.hip's backward_pair with the f loop replaced.
template <int DT, int WD, bool LEAKY, bool TRANSPOSED, bool DROP>
__device__ __forceinline__ float2 backward_pair(GESPMM_GBG_PTRS, int W, int seg, int lo, int d, int h, int H, int F, int l, int q, bool two,
                                                float slope, const DropWords& dw) {
    const int dm = wave_max_degree_w(d, W);
    if (dm == 0) return make_float2(0.0f, 0.0f);
    const int sw = seg * H + h;  // the pair's word (M H, K H, M H F and K H F <= kSddmmMaxNnz: 32-bit word positions)
    const int fo = sw * F;
    float el_s = 0.0f, er_s = 0.0f;
    float2 ms_s = make_float2(0.0f, 1.0f);
    if constexpr (TRANSPOSED) {
        er_s = er[sw];
    } else {
        el_s = el[sw];
        ms_s = stats[sw];  // one 8-byte load
    }
    float w[IT], g[IT], f[IT], dl[IT];
    auto batch = [&](int k0) {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            w[it] = g[it] = dl[it] = 0.0f;
            f[it] = 1.0f;
            if ((k0 + it) * W < dm) {  // wave-uniform
                const int p = l + (k0 + it) * W;
                const int j = ind[lo + (p < d ? p : 0)];
                const int nw = j * H + h;
                uint32_t mb = 0;  // (DROP only) the mask's bits of the entry
                if constexpr (DROP)
                    mb = edge_dropout_bits(dw.s0, dw.s1, (uint32_t)(TRANSPOSED ? j : seg), (uint32_t)(TRANSPOSED ? seg : j), (uint32_t)h);
                float x;
                if constexpr (TRANSPOSED) {
                    const float el_j = el[nw];
                    w[it] = gat_weight(el_j, er_s, stats[nw], slope);
                    dl[it] = delta[nw];
                    x = el_j + er_s;
                } else {
                    const float er_j = er[nw];
                    w[it] = gat_weight(el_s, er_j, ms_s, slope);
                    x = el_s + er_j;
                }
                if constexpr (LEAKY) f[it] = x >= 0.0f ? 1.0f : slope;
                g[it] = group_dots<DT, WD>(fixed, gathered, fo, nw * F, p < d, F, q, two);
                if constexpr (DROP) g[it] = edge_dropout_apply(g[it], mb, dw.threshold, dw.scale);
            }
        }
    };
    const int nt = (dm + W - 1) / W;  // wave-uniform
    float dot = 0.0f, rs = 0.0f;
    if constexpr (TRANSPOSED) {  // one sweep, both regimes: delta is an input
        for (int k0 = 0; k0 < nt; k0 += IT) {
            batch(k0);
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                float r = w[it] * (g[it] - dl[it]);
                if constexpr (LEAKY) r *= f[it];
                rs += (l + (k0 + it) * W < d) ? r : 0.0f;
            }
        }
    } else if (dm <= IT * W) {  // registers: one gather gives delta and grad_el
        batch(0);
#pragma unroll
        for (int it = 0; it < IT; ++it) dot = (l + it * W < d) ? fmaf(w[it], g[it], dot) : dot;
        dot = group_sum_w(dot, W);
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            float r = w[it] * (g[it] - dot);
            if constexpr (LEAKY) r *= f[it];
            rs += (l + it * W < d) ? r : 0.0f;
        }
    } else {  // two sweeps, the second computing w and g again
        for (int k0 = 0; k0 < nt; k0 += IT) {
            batch(k0);
#pragma unroll
            for (int it = 0; it < IT; ++it) dot = (l + (k0 + it) * W < d) ? fmaf(w[it], g[it], dot) : dot;
        }
        dot = group_sum_w(dot, W);
        for (int k0 = 0; k0 < nt; k0 += IT) {
            batch(k0);
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                float r = w[it] * (g[it] - dot);
                if constexpr (LEAKY) r *= f[it];
                rs += (l + (k0 + it) * W < d) ? r : 0.0f;
            }
        }
    }
    rs = group_sum_w(rs, W);
    return make_float2(dot, rs);
}

// out_delta: [S, H] in the row pass (null in the column pass); out_grad: grad_el [M, H] or grad_er [K, H]. Every word written.
// W (4 / 8 / 16) and wsh = log2 W are kernel arguments: wave-uniform.
template <int DT, int WD, bool LEAKY, bool TRANSPOSED, bool DROP>
__device__ __forceinline__ void gat_backward_group_body(const int32_t* __restrict__ ptr, GESPMM_GBG_PTRS, float* __restrict__ out_delta,
                                                        float* __restrict__ out_grad, int S, int H, int F, int rpw, int L, float slope,
                                                        int W, int wsh, const EdgeDropout& drop) {
    const int G = 64 >> wsh;
    DropWords dw = {0u, 0u, 0u, 1.0f};
    if constexpr (DROP) dw = {drop.seed[0], drop.seed[1], drop.threshold, drop.scale};  // wave-uniform loads
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane >> wsh;
    const int l = lane & (W - 1);
    const int q = lane & (WD - 1);
    const bool two = F > 4 * WD;                        // kernel argument: wave-uniform
    const int s0 = (blockIdx.x * kWaves + wave) * rpw;  // (S <= kEdgeSoftmaxMaxRows: no overflow in the last workgroup)
    if (s0 >= S) return;                                // whole wavefront
    const int ns = (S - s0 < rpw) ? S - s0 : rpw;       // segments of this wavefront, 1 .. 63
    const int sp = ptr[s0 + (lane < ns ? lane : ns)];   // lane i: ptr[s0 + i], i <= ns (later lanes repeat the last one)
    const int npairs = ns * H;                          // <= max(64, H)
    const int next = __shfl(sp, lane < 63 ? lane + 1 : 63, 64);
    const bool hubs = __ballot(lane < ns && next - sp > L) != 0;  // wave-uniform
    // ---- segments of at most L entries: the G lane groups take consecutive pairs
    for (int tb = 0; tb < npairs; tb += G) {
        const int t = tb + g;
        const bool act = t < npairs;
        const unsigned tc = act ? (unsigned)t : 0u;
        const int si = (int)(tc / (unsigned)H);  // the pair's segment within the wavefront (an idle group: segment 0, head 0)
        const int h = (int)(tc - (unsigned)si * (unsigned)H);
        int lo = __shfl(sp, si, 64);
        int d = __shfl(sp, si + 1, 64) - lo;
        const bool mine = act && d <= L;  // (an empty segment included: its words are +0)
        if (!act || d <= 0 || d > L) {
            d = 0;
            lo = 0;
        }
        const float2 r = backward_pair<DT, WD, LEAKY, TRANSPOSED, DROP>(GESPMM_GBG_ARGS, W, s0 + si, lo, d, h, H, F, l, q, two, slope, dw);
        if (mine && l == 0) {
            if constexpr (!TRANSPOSED) out_delta[(s0 + si) * H + h] = r.x;
            out_grad[(s0 + si) * H + h] = r.y;
        }
    }
    // ---- hub segments: a whole wavefront per pair (wave-uniform branch: sp lives in lanes, the segment index is a loop counter)
    if (hubs) {
        for (int i = 0; i < ns; ++i) {
            const int lo = __builtin_amdgcn_readlane(sp, i);
            const int d = __builtin_amdgcn_readlane(sp, i + 1) - lo;
            if (d > L)
                for (int h = 0; h < H; ++h) {
                    const float2 r = backward_pair<DT, WD, LEAKY, TRANSPOSED, DROP>(GESPMM_GBG_ARGS, 64, s0 + i, lo, d, h, H, F, lane, q, two, slope, dw);
                    if (lane == 0) {
                        if constexpr (!TRANSPOSED) out_delta[(s0 + i) * H + h] = r.x;
                        out_grad[(s0 + i) * H + h] = r.y;
                    }
                }
        }
    }
}

template <int DT, int WD, bool LEAKY, bool TRANSPOSED>
__global__ __launch_bounds__(kThreads) void gat_backward_group_kernel(const int32_t* __restrict__ ptr, GESPMM_GBG_PTRS,
                                                                       float* __restrict__ out_delta, float* __restrict__ out_grad, int S, int H,
                                                                       int F, int rpw, int L, float slope, int W, int wsh) {
    gat_backward_group_body<DT, WD, LEAKY, TRANSPOSED, false>(ptr, GESPMM_GBG_ARGS, out_delta, out_grad, S, H, F, rpw, L, slope, W, wsh, EdgeDropout{});
}

template <int DT, int WD, bool LEAKY, bool TRANSPOSED>
__global__ __launch_bounds__(kThreads) void gat_backward_group_dropout_kernel(const int32_t* __restrict__ ptr, GESPMM_GBG_PTRS,
                                                                               float* __restrict__ out_delta, float* __restrict__ out_grad,
                                                                               int S, int H, int F, int rpw, int L, float slope, int W, int wsh,
                                                                               EdgeDropout drop) {
    gat_backward_group_body<DT, WD, LEAKY, TRANSPOSED, true>(ptr, GESPMM_GBG_ARGS, out_delta, out_grad, S, H, F, rpw, L, slope, W, wsh, drop);
}

template <int DT, bool LEAKY, bool TRANSPOSED>
hipError_t launch_wd(const int32_t* ptr, const int32_t* ind, const float* el, const float* er, const float* stats, const float* delta,
                     const gb_elem_t<DT>* fixed, const gb_elem_t<DT>* gathered, float* out_delta, float* out_grad, int S, int H, int F, float slope,
                     const GatBackwardLaunch& r, const EdgeDropout* drop, hipStream_t st) {
    const int nblk = (int)(((int64_t)S + kWaves * r.rpw - 1) / (kWaves * r.rpw));
    const int wsh = r.W == 4 ? 2 : r.W == 8 ? 3 : 4;
#define GESPMM_GBG(WW)                                                                                                                    \
    case WW:                                                                                                                              \
        if (drop) {                                                                                                                       \
            hipLaunchKernelGGL((gat_backward_group_dropout_kernel<DT, WW, LEAKY, TRANSPOSED>), dim3(nblk), dim3(kThreads), 0, st, ptr, ind, el, \
                               er, reinterpret_cast<const float2*>(stats), delta, fixed, gathered, out_delta, out_grad, S, H, F, r.rpw,  \
                               r.L, slope, r.W, wsh, *drop);                                                                              \
            return hipGetLastError();                                                                                                     \
        }                                                                                                                                 \
        hipLaunchKernelGGL((gat_backward_group_kernel<DT, WW, LEAKY, TRANSPOSED>), dim3(nblk), dim3(kThreads), 0, st, ptr, ind, el, er,       \
                           reinterpret_cast<const float2*>(stats), delta, fixed, gathered, out_delta, out_grad, S, H, F, r.rpw, r.L,     \
                           slope, r.W, wsh);                                                                                              \
        return hipGetLastError();
    switch (r.Wd) {
        GESPMM_GBG(4)
        GESPMM_GBG(8)
        GESPMM_GBG(16)
        GESPMM_GBG(32)
        GESPMM_GBG(64)
    }
#undef GESPMM_GBG
    return hipErrorInvalidValue;
}

bool dense_words_fit(int64_t rows, int64_t H, int64_t F) { return H >= 1 && F >= 1 && rows <= kSddmmMaxNnz / H / F; }

// What the kernel relies on: the lane form's limits, and the form rule's own conditions (the caller asked resolve_gat_backward or
// resolve_gat_backward_x16: one 4-element vector's bytes — 16, or 8 at 16 bits — divide both addresses; a
// launch that does not meet them is refused, never served by other loads).
template <int DT>
bool launchable(int64_t S, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, const gb_elem_t<DT>* a, const gb_elem_t<DT>* b,
                const GatBackwardLaunch& r) {
    return r.form == kGatBackwardGroup && r.V == 4 && F % 4 == 0 && F >= 16 && F <= kGatBackwardGroupMaxF && 8 * (int64_t)r.Wd >= F &&
           (reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) % (4 * sizeof(gb_elem_t<DT>)) == 0 &&
           (r.W == 4 || r.W == 8 || r.W == 16) && S >= 1 && S <= kEdgeSoftmaxMaxRows && M >= 1 && K >= 1 && H >= 1 && nnz >= 1 &&
           nnz <= kSddmmMaxNnz / H && dense_words_fit(M, H, F) && dense_words_fit(K, H, F) && r.rpw >= 1 && r.rpw <= 63 &&
           (int64_t)r.rpw * H <= (H > 64 ? H : 64) && r.L >= 1;
}

// The two passes as the entry points take them (nnz >= 1).
template <int DT>
hipError_t group_el(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, const float* stats,
                    const gb_elem_t<DT>* grad_out, const gb_elem_t<DT>* feat, float* delta, float* grad_el, int64_t M, int64_t K, int64_t H,
                    int64_t F, int64_t nnz, float slope, const GatBackwardLaunch& r, const EdgeDropout* drop, hipStream_t st) {
    if (!launchable<DT>(M, M, K, H, F, nnz, grad_out, feat, r) || (drop && !drop->seed)) return hipErrorInvalidValue;
    if (slope != 1.0f)
        return launch_wd<DT, true, false>(rowptr, colind, el, er, stats, nullptr, grad_out, feat, delta, grad_el, (int)M, (int)H, (int)F, slope, r, drop, st);
    return launch_wd<DT, false, false>(rowptr, colind, el, er, stats, nullptr, grad_out, feat, delta, grad_el, (int)M, (int)H, (int)F, slope, r, drop, st);
}

template <int DT>
hipError_t group_er(const int32_t* colptr, const int32_t* rowind, const float* el, const float* er, const float* stats, const float* delta,
                    const gb_elem_t<DT>* grad_out, const gb_elem_t<DT>* feat, float* grad_er, int64_t M, int64_t K, int64_t H, int64_t F,
                    int64_t nnz, float slope, const GatBackwardLaunch& r, const EdgeDropout* drop, hipStream_t st) {
    if (!launchable<DT>(K, M, K, H, F, nnz, grad_out, feat, r) || (drop && !drop->seed)) return hipErrorInvalidValue;
    if (slope != 1.0f)
        return launch_wd<DT, true, true>(colptr, rowind, el, er, stats, delta, feat, grad_out, nullptr, grad_er, (int)K, (int)H, (int)F, slope, r, drop, st);
    return launch_wd<DT, false, true>(colptr, rowind, el, er, stats, delta, feat, grad_out, nullptr, grad_er, (int)K, (int)H, (int)F, slope, r, drop, st);
}

}  // namespace
}  // namespace gespmm
