// edge_softmax.hip — the edge softmax over CSR rows and its backward on fp32 (gfx950). Contract, lane geometry and the pinned
// summation order: edge_softmax.h.
//
// Safety rules this file keeps: every load of rowptr / score / alpha / grad_alpha is clamped to a valid position (a lane past its
// row's end re-reads the row's first entry, a lane group without a pair reads word h of entry 0) and dropped by a select; loop trip
// counts and the register / sweep choice are wave-uniform (made so with readfirstlane), so no load and no cross-lane move sits under a
// divergent branch; only stores are predicated. A wavefront past M returns whole.

#include "edge_softmax.h"

#include <math.h>

#include "spmm_kernels.h"

namespace gespmm {
namespace {

constexpr int IT = kEdgeSoftmaxIT;  // entries a lane keeps in registers

template <int W>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int m = W >> 1; m > 0; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

template <int W>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int m = W >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// Largest degree among the wavefront's 64 / W lane groups, in a scalar register.
template <int W>
__device__ __forceinline__ int wave_max_degree(int d) {
#pragma unroll
    for (int m = 32; m >= W; m >>= 1) {
        const int o = __shfl_xor(d, m, 64);
        d = o > d ? o : d;
    }
    return __builtin_amdgcn_readfirstlane(d);
}

template <bool LEAKY>
__device__ __forceinline__ float leaky(float x, float slope) {
    if constexpr (LEAKY) return x >= 0.0f ? x : slope * x;
    return x;
}

// One (row, head) pair per lane group: the row's d entries start at entry lo, lane l of the W takes entries l + t W. All 64 lanes
// arrive together; d is uniform in the group, d == 0 (then lo == 0) means the group has nothing to do and only keeps the others company.
template <int W, bool LEAKY>
__device__ __forceinline__ void softmax_pair(const float* __restrict__ score, float* __restrict__ out, int lo, int d, int h, int H, int l,
                                             float slope) {
    const int dm = wave_max_degree<W>(d);
    if (dm == 0) return;
    auto word = [&](int p) { return (lo + (p < d ? p : 0)) * H + h; };  // (nnz H <= kSddmmMaxNnz: 32-bit word positions)
    if (dm <= IT * W) {
        float x[IT], t[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            x[it] = -INFINITY;
            if (it * W < dm) {  // wave-uniform
                const int p = l + it * W;
                const float v = score[word(p)];
                x[it] = p < d ? leaky<LEAKY>(v, slope) : -INFINITY;
            }
        }
        float m = -INFINITY;
#pragma unroll
        for (int it = 0; it < IT; ++it) m = fmaxf(m, x[it]);
        m = group_max<W>(m);
        float s = 0.0f;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            t[it] = (l + it * W < d) ? __expf(x[it] - m) : 0.0f;  // (s + 0 == s: the chain of the sweep below)
            s += t[it];
        }
        s = group_sum<W>(s);
#pragma unroll
        for (int it = 0; it < IT; ++it)
            if (l + it * W < d) out[word(l + it * W)] = t[it] / s;
    } else {
        const int nt = (dm + W - 1) / W;  // wave-uniform
        float m = -INFINITY;
#pragma unroll 4
        for (int k = 0; k < nt; ++k) {
            const int p = l + k * W;
            const float v = score[word(p)];
            m = fmaxf(m, p < d ? leaky<LEAKY>(v, slope) : -INFINITY);
        }
        m = group_max<W>(m);
        float s = 0.0f;
#pragma unroll 4
        for (int k = 0; k < nt; ++k) {
            const int p = l + k * W;
            const float v = score[word(p)];
            s += p < d ? __expf(leaky<LEAKY>(v, slope) - m) : 0.0f;
        }
        s = group_sum<W>(s);
#pragma unroll 4
        for (int k = 0; k < nt; ++k) {
            const int p = l + k * W;
            const float v = score[word(p)];
            if (p < d) out[word(p)] = __expf(leaky<LEAKY>(v, slope) - m) / s;
        }
    }
}

template <int W, bool LEAKY>
__device__ __forceinline__ void softmax_backward_pair(const float* __restrict__ alpha, const float* __restrict__ galpha,
                                                      const float* __restrict__ score, float* __restrict__ grad, int lo, int d, int h,
                                                      int H, int l, float slope) {
    const int dm = wave_max_degree<W>(d);
    if (dm == 0) return;
    auto word = [&](int p) { return (lo + (p < d ? p : 0)) * H + h; };
    if (dm <= IT * W) {
        float a[IT], g[IT], f[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            a[it] = g[it] = 0.0f;
            f[it] = 1.0f;
            if (it * W < dm) {  // wave-uniform
                const int w = word(l + it * W);
                a[it] = alpha[w];
                g[it] = galpha[w];
                if constexpr (LEAKY) f[it] = score[w] >= 0.0f ? 1.0f : slope;
            }
        }
        float dot = 0.0f;
#pragma unroll
        for (int it = 0; it < IT; ++it) dot = (l + it * W < d) ? fmaf(a[it], g[it], dot) : dot;
        dot = group_sum<W>(dot);
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            float r = a[it] * (g[it] - dot);
            if constexpr (LEAKY) r *= f[it];
            if (l + it * W < d) grad[word(l + it * W)] = r;
        }
    } else {
        const int nt = (dm + W - 1) / W;  // wave-uniform
        float dot = 0.0f;
#pragma unroll 4
        for (int k = 0; k < nt; ++k) {
            const int p = l + k * W;
            const int w = word(p);
            const float av = alpha[w], gv = galpha[w];
            dot = p < d ? fmaf(av, gv, dot) : dot;
        }
        dot = group_sum<W>(dot);
#pragma unroll 4
        for (int k = 0; k < nt; ++k) {
            const int p = l + k * W;
            const int w = word(p);
            const float av = alpha[w], gv = galpha[w];
            float r = av * (gv - dot);
            if constexpr (LEAKY) r *= score[w] >= 0.0f ? 1.0f : slope;
            if (p < d) grad[w] = r;
        }
    }
}

// forward: in0 = score, out = the softmax. backward: in0 = alpha, in1 = grad_alpha, in2 = score (LEAKY only), out = grad_score.
template <int W, bool LEAKY, bool BWD>
__device__ __forceinline__ void pair(const float* __restrict__ in0, const float* __restrict__ in1, const float* __restrict__ in2,
                                     float* __restrict__ out, int lo, int d, int h, int H, int l, float slope) {
    if constexpr (BWD) softmax_backward_pair<W, LEAKY>(in0, in1, in2, out, lo, d, h, H, l, slope);
    else softmax_pair<W, LEAKY>(in0, out, lo, d, h, H, l, slope);
}

template <int W, bool LEAKY, bool BWD>
__global__ __launch_bounds__(kThreads) void edge_softmax_kernel(const int32_t* __restrict__ rowptr, const float* __restrict__ in0,
                                                                 const float* __restrict__ in1, const float* __restrict__ in2,
                                                                 float* __restrict__ out, int M, int H, int rpw, int L, float slope) {
    constexpr int G = 64 / W;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / W;
    const int l = lane % W;
    const int r0 = (blockIdx.x * kWaves + wave) * rpw;  // (M <= kEdgeSoftmaxMaxRows: no overflow in the last workgroup)
    if (r0 >= M) return;                                 // whole wavefront
    const int nr = (M - r0 < rpw) ? M - r0 : rpw;        // rows of this wavefront, 1 .. 63
    const int rp = rowptr[r0 + (lane < nr ? lane : nr)];  // lane i: rowptr[r0 + i], i <= nr (later lanes repeat the last one)
    const int npairs = nr * H;                            // <= max(64, H)
    const int next = __shfl(rp, lane < 63 ? lane + 1 : 63, 64);
    const bool hubs = __ballot(lane < nr && next - rp > L) != 0;  // wave-uniform
    // ---- rows of at most L entries: the G lane groups take consecutive pairs
    for (int tb = 0; tb < npairs; tb += G) {
        const int t = tb + g;
        const bool act = t < npairs;
        const unsigned tc = act ? (unsigned)t : 0u;
        const int er = (int)(tc / (unsigned)H);
        const int h = (int)(tc - (unsigned)er * (unsigned)H);
        int lo = __shfl(rp, er, 64);
        int d = __shfl(rp, er + 1, 64) - lo;
        if (!act || d <= 0 || d > L) {
            d = 0;
            lo = 0;
        }
        pair<W, LEAKY, BWD>(in0, in1, in2, out, lo, d, h, H, l, slope);
    }
    // ---- hub rows: a whole wavefront per pair (wave-uniform branch: rp lives in lanes, the row index is a loop counter)
    if (hubs) {
        for (int i = 0; i < nr; ++i) {
            const int lo = __builtin_amdgcn_readlane(rp, i);
            const int d = __builtin_amdgcn_readlane(rp, i + 1) - lo;
            if (d > L)
                for (int h = 0; h < H; ++h) pair<64, LEAKY, BWD>(in0, in1, in2, out, lo, d, h, H, lane, slope);
        }
    }
}

template <bool LEAKY, bool BWD>
hipError_t launch_w(const int32_t* rowptr, const float* in0, const float* in1, const float* in2, float* out, int M, int H, float slope,
                    const EdgeSoftmaxLaunch& r, hipStream_t st) {
    const int nblk = (int)(((int64_t)M + kWaves * r.rpw - 1) / (kWaves * r.rpw));
#define GESPMM_ES(WW)                                                                                                              \
    case WW:                                                                                                                        \
        hipLaunchKernelGGL((edge_softmax_kernel<WW, LEAKY, BWD>), dim3(nblk), dim3(kThreads), 0, st, rowptr, in0, in1, in2, out, M, H, \
                           r.rpw, r.L, slope);                                                                                      \
        return hipGetLastError();
    switch (r.W) {
        GESPMM_ES(4)
        GESPMM_ES(8)
        GESPMM_ES(16)
    }
#undef GESPMM_ES
    return hipErrorInvalidValue;
}

bool launchable(int64_t M, int64_t H, int64_t nnz, const EdgeSoftmaxLaunch& r) {
    return M >= 1 && M <= kEdgeSoftmaxMaxRows && H >= 1 && nnz >= 1 && nnz <= kSddmmMaxNnz / H && r.rpw >= 1 && r.rpw <= 63 &&
           (int64_t)r.rpw * H <= (H > 64 ? H : 64) && r.L >= 1;
}

}  // namespace

hipError_t launch_edge_softmax(const int32_t* rowptr, const float* score, float* out, int64_t M, int64_t H, int64_t nnz, float slope,
                               const EdgeSoftmaxLaunch& r, hipStream_t st) {
    if (nnz == 0 || M == 0) return hipSuccess;
    if (!launchable(M, H, nnz, r)) return hipErrorInvalidValue;
    if (slope != 1.0f) return launch_w<true, false>(rowptr, score, nullptr, nullptr, out, (int)M, (int)H, slope, r, st);
    return launch_w<false, false>(rowptr, score, nullptr, nullptr, out, (int)M, (int)H, slope, r, st);
}

hipError_t launch_edge_softmax_backward(const int32_t* rowptr, const float* alpha, const float* grad_alpha, const float* score,
                                        float* grad_score, int64_t M, int64_t H, int64_t nnz, float slope, const EdgeSoftmaxLaunch& r,
                                        hipStream_t st) {
    if (nnz == 0 || M == 0) return hipSuccess;
    if (!launchable(M, H, nnz, r)) return hipErrorInvalidValue;
    if (slope != 1.0f) return launch_w<true, true>(rowptr, alpha, grad_alpha, score, grad_score, (int)M, (int)H, slope, r, st);
    return launch_w<false, true>(rowptr, alpha, grad_alpha, nullptr, grad_score, (int)M, (int)H, slope, r, st);
}

}  // namespace gespmm
