// gatv2_attention.hip — fused GATv2 attention over a sparsity pattern and its backward on fp32 operands (gfx950). Contract, geometry,
// pinned orders and safety rules: gatv2_attention.h.
//
//     s_p = sum_f att[h, f] leaky(xl[r, h, f] + xr[c, h, f])      a_p = exp(s_p - m) / l      out[r, h, :] = sum_p a_p xr[c, h, :]

#include "gatv2_attention.h"

#include "spmm_kernels.h"

namespace gespmm {

namespace {

template <int V> struct GaVec;
template <> struct GaVec<1> { using type = float; };
template <> struct GaVec<2> { using type = float __attribute__((ext_vector_type(2))); };
template <> struct GaVec<4> { using type = float __attribute__((ext_vector_type(4))); };

template <int V> __device__ __forceinline__ float ga_get(const typename GaVec<V>::type& x, int i) {
    if constexpr (V == 1) return x;
    else return x[i];
}
template <int V> __device__ __forceinline__ void ga_set(typename GaVec<V>::type& x, int i, float v) {
    if constexpr (V == 1) x = v;
    else x[i] = v;
}

// The seed's two words and the two kernel arguments of a dropout launch (wave-uniform).
struct GaDrop {
    uint32_t s0, s1, threshold;
    float scale;
};

// What a lane group knows about its pair.
struct GaPair {
    int pair;   // segment * H + h, clamped to the last pair for an idle group
    int seg, h;
    int lo, d;  // the segment's entries [lo, lo + d); d == 0 for an idle group
    int dmax;   // the longest segment among the wavefront's groups (wave-uniform)
    bool live;
};

__device__ __forceinline__ GaPair ga_pair(const int32_t* __restrict__ ptr, int pair0, int g, int P, int H) {
    GaPair p;
    p.live = pair0 + g < P;  // an idle group walks the last pair as an empty one and stores nothing
    p.pair = p.live ? pair0 + g : P - 1;
    p.seg = p.pair / H;
    p.h = p.pair - p.seg * H;
    p.lo = ptr[p.seg];
    p.d = p.live ? ptr[p.seg + 1] - p.lo : 0;
    int dmax = p.d;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const int o = __shfl_xor(dmax, m, 64);
        dmax = o > dmax ? o : dmax;
    }
    p.dmax = __builtin_amdgcn_readfirstlane(dmax);
    return p;
}

// The lane's NT vectors of the head slice that starts at `base`: a vector past the slice is clamped to the slice's first word and
// replaced by zeros. nT = ceil(F / (W V)) is wave-uniform.
template <int V, int W, int NT>
__device__ __forceinline__ void ga_load(const float* __restrict__ base, int l, int F, int nT, typename GaVec<V>::type (&x)[NT]) {
    using T = typename GaVec<V>::type;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        x[t] = T{};
        if (t < nT) {
            const int j = l * V + t * W * V;
            const bool in = j < F;  // (V divides F: a vector is inside the slice or past it, whole)
            const T y = *reinterpret_cast<const T*>(base + (in ? j : 0));
#pragma unroll
            for (int i = 0; i < V; ++i) ga_set<V>(x[t], i, in ? ga_get<V>(y, i) : 0.0f);
        }
    }
}

// leaky(t) = t >= 0 ? t : slope * t. `leaky` is false for slope == 1: no multiply. (The expression of gatv2_score.hip.)
__device__ __forceinline__ float ga_leaky(float t, float slope, bool leaky) { return (leaky && !(t >= 0.0f)) ? slope * t : t; }

// The lane's chain of the pinned dot (before the butterfly).
template <int V, int NT>
__device__ __forceinline__ float ga_chain(const typename GaVec<V>::type (&x)[NT], const typename GaVec<V>::type (&y)[NT], int nT) {
    float acc = 0.0f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t < nT) {
#pragma unroll
            for (int i = 0; i < V; ++i) acc = __builtin_fmaf(ga_get<V>(x[t], i), ga_get<V>(y[t], i), acc);
        }
    }
    return acc;
}

// The lane's chain of the score: fmaf(att_j, leaky(fl(x_j + y_j)), acc). A lane past the slice holds zeros in all three: fmaf(0, 0, acc).
template <int V, int NT>
__device__ __forceinline__ float ga_score_chain(const typename GaVec<V>::type (&a)[NT], const typename GaVec<V>::type (&x)[NT],
                                                const typename GaVec<V>::type (&y)[NT], int nT, float slope, bool leaky) {
    float acc = 0.0f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t < nT) {
#pragma unroll
            for (int i = 0; i < V; ++i)
                acc = __builtin_fmaf(ga_get<V>(a[t], i), ga_leaky(ga_get<V>(x[t], i) + ga_get<V>(y[t], i), slope, leaky), acc);
        }
    }
    return acc;
}

template <int W> __device__ __forceinline__ float ga_butterfly(float x) {
#pragma unroll
    for (int m = W >> 1; m > 0; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

template <int V, int W, int NT>
__device__ __forceinline__ void ga_store(float* __restrict__ base, int l, int F, int nT, const typename GaVec<V>::type (&x)[NT]) {
    using T = typename GaVec<V>::type;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t < nT) {
            const int j = l * V + t * W * V;
            if (j < F) *reinterpret_cast<T*>(base + j) = x[t];
        }
    }
}

// W indices of the group's segment, one per lane: a lane past its segment re-reads the segment's first entry (entry 0 where the segment
// is empty: nnz >= 1); what is gathered through it is dropped by a select.
__device__ __forceinline__ int ga_index(const int32_t* __restrict__ ind, const GaPair& p, int pe) {
    return ind[pe < p.d ? p.lo + pe : (p.d > 0 ? p.lo : 0)];
}

constexpr int kGaUnrollRow = 4;  // entries whose ONE gathered row is in flight per lane group: forward and row pass (W is a multiple)
constexpr int kGaUnrollCol = 2;  // entries whose TWO gathered rows (and three words) are in flight per lane group: column pass

// ---- forward
template <int V, int W, bool DROP>
__global__ __launch_bounds__(kThreads) void gatv2_attention_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                                    const float* __restrict__ xl, const float* __restrict__ xr,
                                                                    const float* __restrict__ att, float* __restrict__ out,
                                                                    float* __restrict__ stats, int M, int H, int F, float slope,
                                                                    int leaky_i, EdgeDropout drop) {
    constexpr int G = 64 / W;
    constexpr int NT = 8 / V;
    constexpr int UG = kGaUnrollRow;
    using T = typename GaVec<V>::type;
    const bool leaky = leaky_i != 0;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / W;
    const int l = lane % W;
    const int P = M * H;  // (M H F <= kSddmmMaxNnz: 32-bit word positions)
    const int pair0 = (blockIdx.x * kWaves + wave) * G;
    if (pair0 >= P) return;  // whole wavefront
    GaDrop dw = {};
    if constexpr (DROP) dw = {drop.seed[0], drop.seed[1], drop.threshold, drop.scale};  // wave-uniform loads
    const GaPair p = ga_pair(rowptr, pair0, g, P, H);
    const int nT = (F + W * V - 1) / (W * V);
    const int ld = H * F;
    const int off = p.h * F;
    T xs[NT], as[NT], acc[NT];
    ga_load<V, W, NT>(xl + p.pair * F, l, F, nT, xs);
    ga_load<V, W, NT>(att + off, l, F, nT, as);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = T{};
    float m = 0.0f, lsum = 0.0f;
    for (int p0 = 0; p0 < p.dmax; p0 += W) {
        const int c = ga_index(colind, p, p0 + l);
        const int kmax = (p.dmax - p0 < W) ? p.dmax - p0 : W;
        for (int k0 = 0; k0 < kmax; k0 += UG) {
            T xv[UG][NT];
            int ck[UG];
#pragma unroll
            for (int u = 0; u < UG; ++u) {  // (W is a multiple of UG: k0 + u < W)
                ck[u] = __shfl(c, k0 + u, W);
                ga_load<V, W, NT>(xr + ck[u] * ld + off, l, F, nT, xv[u]);
            }
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                const int e = p0 + k0 + u;
                const bool valid = e < p.d;
                const float s = ga_butterfly<W>(ga_score_chain<V, NT>(as, xs, xv[u], nT, slope, leaky));
                const float mo = e == 0 ? s : m;  // the first entry: c = t = __expf(0) = 1, l = 1, acc = xr
                const float mn = fmaxf(mo, s);
                const float cc = __expf(mo - mn);
                const float te = __expf(s - mn);
                const float ln = __builtin_fmaf(lsum, cc, te);
                float tv = te;
                if constexpr (DROP)
                    tv = edge_dropout_apply(te, edge_dropout_bits(dw.s0, dw.s1, (uint32_t)p.seg, (uint32_t)ck[u], (uint32_t)p.h), dw.threshold,
                                            dw.scale);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
#pragma unroll
                    for (int i = 0; i < V; ++i) {
                        const float a = ga_get<V>(acc[t], i);
                        const float an = __builtin_fmaf(tv, ga_get<V>(xv[u][t], i), a * cc);
                        ga_set<V>(acc[t], i, valid ? an : a);
                    }
                }
                m = valid ? mn : m;
                lsum = valid ? ln : lsum;
            }
        }
    }
    const bool some = p.d > 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int i = 0; i < V; ++i) ga_set<V>(acc[t], i, some ? ga_get<V>(acc[t], i) / lsum : 0.0f);
    }
    if (p.live) {
        ga_store<V, W, NT>(out + p.pair * F, l, F, nT, acc);
        if (l == 0) *reinterpret_cast<float2*>(stats + 2 * p.pair) = make_float2(m, lsum);
    }
}

// ---- backward, row pass
template <int V, int W, bool DROP, bool PART>
__global__ __launch_bounds__(kThreads) void gatv2_attention_backward_row_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind, const float* __restrict__ xl, const float* __restrict__ xr,
    const float* __restrict__ att, const float* __restrict__ stats, const float* __restrict__ out, const float* __restrict__ grad_out,
    float* __restrict__ delta, float* __restrict__ grad_xl, float* __restrict__ att_part, int M, int H, int F, float slope, int leaky_i,
    EdgeDropout drop) {
    constexpr int G = 64 / W;
    constexpr int NT = 8 / V;
    constexpr int UG = kGaUnrollRow;
    using T = typename GaVec<V>::type;
    const bool leaky = leaky_i != 0;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / W;
    const int l = lane % W;
    const int P = M * H;
    const int pair0 = (blockIdx.x * kWaves + wave) * G;
    if (pair0 >= P) return;  // whole wavefront
    GaDrop dw = {};
    if constexpr (DROP) dw = {drop.seed[0], drop.seed[1], drop.threshold, drop.scale};
    const GaPair p = ga_pair(rowptr, pair0, g, P, H);
    const int nT = (F + W * V - 1) / (W * V);
    const int ld = H * F;
    const int off = p.h * F;
    T xs[NT], as[NT], gs[NT], acc_x[NT], acc_a[NT];
    float dl;
    {
        T os[NT];
        ga_load<V, W, NT>(grad_out + p.pair * F, l, F, nT, gs);
        ga_load<V, W, NT>(out + p.pair * F, l, F, nT, os);
        dl = ga_butterfly<W>(ga_chain<V, NT>(gs, os, nT));
    }
    ga_load<V, W, NT>(xl + p.pair * F, l, F, nT, xs);
    ga_load<V, W, NT>(att + off, l, F, nT, as);
    const float2 ml = *reinterpret_cast<const float2*>(stats + 2 * p.pair);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        acc_x[t] = T{};
        acc_a[t] = T{};
    }
    for (int p0 = 0; p0 < p.dmax; p0 += W) {
        const int c = ga_index(colind, p, p0 + l);
        const int kmax = (p.dmax - p0 < W) ? p.dmax - p0 : W;
        for (int k0 = 0; k0 < kmax; k0 += UG) {
            T xv[UG][NT];
            int ck[UG];
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                ck[u] = __shfl(c, k0 + u, W);
                ga_load<V, W, NT>(xr + ck[u] * ld + off, l, F, nT, xv[u]);
            }
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                const bool valid = p0 + k0 + u < p.d;
                const float s = ga_butterfly<W>(ga_score_chain<V, NT>(as, xs, xv[u], nT, slope, leaky));
                float gp = ga_butterfly<W>(ga_chain<V, NT>(gs, xv[u], nT));
                if constexpr (DROP)
                    gp = edge_dropout_apply(gp, edge_dropout_bits(dw.s0, dw.s1, (uint32_t)p.seg, (uint32_t)ck[u], (uint32_t)p.h), dw.threshold,
                                            dw.scale);
                const float a = __expf(s - ml.x) / ml.y;
                const float ds = a * (gp - dl);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
#pragma unroll
                    for (int i = 0; i < V; ++i) {
                        const float tt = ga_get<V>(xs[t], i) + ga_get<V>(xv[u][t], i);
                        const bool neg = leaky && !(tt >= 0.0f);
                        const float ai = ga_get<V>(as[t], i);
                        const float mf = neg ? ai * slope : ai;
                        const float ox = ga_get<V>(acc_x[t], i);
                        const float nx = __builtin_fmaf(ds, mf, ox);
                        ga_set<V>(acc_x[t], i, valid ? nx : ox);
                        if constexpr (PART) {
                            const float oa = ga_get<V>(acc_a[t], i);
                            const float na = __builtin_fmaf(ds, neg ? slope * tt : tt, oa);
                            ga_set<V>(acc_a[t], i, valid ? na : oa);
                        }
                    }
                }
            }
        }
    }
    if (p.live) {
        ga_store<V, W, NT>(grad_xl + p.pair * F, l, F, nT, acc_x);
        if constexpr (PART) ga_store<V, W, NT>(att_part + p.pair * F, l, F, nT, acc_a);
        if (l == 0) delta[p.pair] = dl;
    }
}

// ---- backward, column pass: segment = column c of the pattern, index = row r
template <int V, int W, bool DROP>
__global__ __launch_bounds__(kThreads) void gatv2_attention_backward_col_kernel(
    const int32_t* __restrict__ colptr, const int32_t* __restrict__ rowind, const float* __restrict__ xl, const float* __restrict__ xr,
    const float* __restrict__ att, const float* __restrict__ stats, const float* __restrict__ delta, const float* __restrict__ grad_out,
    float* __restrict__ grad_xr, int K, int H, int F, float slope, int leaky_i, EdgeDropout drop) {
    constexpr int G = 64 / W;
    constexpr int NT = 8 / V;
    constexpr int UG = kGaUnrollCol;
    using T = typename GaVec<V>::type;
    const bool leaky = leaky_i != 0;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / W;
    const int l = lane % W;
    const int P = K * H;
    const int pair0 = (blockIdx.x * kWaves + wave) * G;
    if (pair0 >= P) return;  // whole wavefront
    GaDrop dw = {};
    if constexpr (DROP) dw = {drop.seed[0], drop.seed[1], drop.threshold, drop.scale};
    const GaPair p = ga_pair(colptr, pair0, g, P, H);
    const int nT = (F + W * V - 1) / (W * V);
    T xs[NT], as[NT], acc1[NT], acc2[NT];
    ga_load<V, W, NT>(xr + p.pair * F, l, F, nT, xs);
    ga_load<V, W, NT>(att + p.h * F, l, F, nT, as);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        acc1[t] = T{};
        acc2[t] = T{};
    }
    for (int p0 = 0; p0 < p.dmax; p0 += W) {
        const int r = ga_index(rowind, p, p0 + l);
        const int kmax = (p.dmax - p0 < W) ? p.dmax - p0 : W;
        for (int k0 = 0; k0 < kmax; k0 += UG) {
            T xv[UG][NT], ov[UG][NT];
            float2 ml[UG];
            float dl[UG];
            int rk[UG];
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                rk[u] = __shfl(r, k0 + u, W);
                const int rp = rk[u] * H + p.h;  // the pair of the entry's row
                ga_load<V, W, NT>(xl + rp * F, l, F, nT, xv[u]);
                ga_load<V, W, NT>(grad_out + rp * F, l, F, nT, ov[u]);
                ml[u] = *reinterpret_cast<const float2*>(stats + 2 * rp);
                dl[u] = delta[rp];
            }
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                const bool valid = p0 + k0 + u < p.d;
                const float s = ga_butterfly<W>(ga_score_chain<V, NT>(as, xv[u], xs, nT, slope, leaky));
                float gp = ga_butterfly<W>(ga_chain<V, NT>(ov[u], xs, nT));
                const float a = __expf(s - ml[u].x) / ml[u].y;
                float av = a;
                if constexpr (DROP) {
                    const uint32_t bits = edge_dropout_bits(dw.s0, dw.s1, (uint32_t)rk[u], (uint32_t)p.seg, (uint32_t)p.h);
                    gp = edge_dropout_apply(gp, bits, dw.threshold, dw.scale);
                    av = edge_dropout_apply(a, bits, dw.threshold, dw.scale);
                }
                const float ds = a * (gp - dl[u]);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
#pragma unroll
                    for (int i = 0; i < V; ++i) {
                        const float tt = ga_get<V>(xv[u][t], i) + ga_get<V>(xs[t], i);
                        const bool neg = leaky && !(tt >= 0.0f);
                        const float ai = ga_get<V>(as[t], i);
                        const float mf = neg ? ai * slope : ai;
                        const float o1 = ga_get<V>(acc1[t], i), o2 = ga_get<V>(acc2[t], i);
                        const float n1 = __builtin_fmaf(ds, mf, o1);
                        const float n2 = __builtin_fmaf(av, ga_get<V>(ov[u][t], i), o2);
                        ga_set<V>(acc1[t], i, valid ? n1 : o1);
                        ga_set<V>(acc2[t], i, valid ? n2 : o2);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int i = 0; i < V; ++i) ga_set<V>(acc1[t], i, ga_get<V>(acc1[t], i) + ga_get<V>(acc2[t], i));
    }
    if (p.live) ga_store<V, W, NT>(grad_xr + p.pair * F, l, F, nT, acc1);
}

// blocks that cover `pairs` (segment, head) pairs with 64 / W lane groups per wavefront
inline int ga_blocks(int64_t pairs, int W) {
    const int64_t per_block = (int64_t)kWaves * (64 / W);
    return (int)((pairs + per_block - 1) / per_block);
}

// One switch over (V, W, dropout) for the three kernels: KERNEL is the template's name and its arguments after (V, W, DROP) — in
// parentheses, with a leading comma, or empty — the rest the kernel's arguments before `drop`.
#define GESPMM_GA_UNWRAP(...) __VA_ARGS__
#define GESPMM_GA_CASE(KERNEL, EXTRA, VV, WW, PAIRS, ...)                                                                                 \
    case VV * 100 + WW:                                                                                                                   \
        if (drop)                                                                                                                         \
            hipLaunchKernelGGL((KERNEL<VV, WW, true GESPMM_GA_UNWRAP EXTRA>), dim3(ga_blocks(PAIRS, WW)), dim3(kThreads), 0, st,          \
                               __VA_ARGS__, *drop);                                                                                       \
        else                                                                                                                              \
            hipLaunchKernelGGL((KERNEL<VV, WW, false GESPMM_GA_UNWRAP EXTRA>), dim3(ga_blocks(PAIRS, WW)), dim3(kThreads), 0, st,         \
                               __VA_ARGS__, EdgeDropout{});                                                                               \
        return hipGetLastError();
#define GESPMM_GA_SWITCH(KERNEL, EXTRA, PAIRS, ...)                     \
    switch (r.V * 100 + r.W) {                                          \
        GESPMM_GA_CASE(KERNEL, EXTRA, 1, 4, PAIRS, __VA_ARGS__)         \
        GESPMM_GA_CASE(KERNEL, EXTRA, 1, 8, PAIRS, __VA_ARGS__)         \
        GESPMM_GA_CASE(KERNEL, EXTRA, 1, 16, PAIRS, __VA_ARGS__)        \
        GESPMM_GA_CASE(KERNEL, EXTRA, 1, 32, PAIRS, __VA_ARGS__)        \
        GESPMM_GA_CASE(KERNEL, EXTRA, 1, 64, PAIRS, __VA_ARGS__)        \
        GESPMM_GA_CASE(KERNEL, EXTRA, 2, 4, PAIRS, __VA_ARGS__)         \
        GESPMM_GA_CASE(KERNEL, EXTRA, 2, 8, PAIRS, __VA_ARGS__)         \
        GESPMM_GA_CASE(KERNEL, EXTRA, 2, 16, PAIRS, __VA_ARGS__)        \
        GESPMM_GA_CASE(KERNEL, EXTRA, 2, 32, PAIRS, __VA_ARGS__)        \
        GESPMM_GA_CASE(KERNEL, EXTRA, 2, 64, PAIRS, __VA_ARGS__)        \
        GESPMM_GA_CASE(KERNEL, EXTRA, 4, 4, PAIRS, __VA_ARGS__)         \
        GESPMM_GA_CASE(KERNEL, EXTRA, 4, 8, PAIRS, __VA_ARGS__)         \
        GESPMM_GA_CASE(KERNEL, EXTRA, 4, 16, PAIRS, __VA_ARGS__)        \
        GESPMM_GA_CASE(KERNEL, EXTRA, 4, 32, PAIRS, __VA_ARGS__)        \
        GESPMM_GA_CASE(KERNEL, EXTRA, 4, 64, PAIRS, __VA_ARGS__)        \
    }                                                                   \
    return hipErrorInvalidValue;

// Sizes the kernels' 32-bit word positions hold, and a launch shape that covers the slice with 8 floats per lane.
bool ga_launchable(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, const Gatv2AttentionLaunch& r, const EdgeDropout* drop) {
    if (nnz < 1 || M < 1 || K < 1 || H < 1 || F < 1 || F > kGatv2AttentionMaxF || !r.supported) return false;
    if (nnz > kSddmmMaxNnz || M > kSddmmMaxNnz / H || K > kSddmmMaxNnz / H || M * H > kSddmmMaxNnz / F || K * H > kSddmmMaxNnz / F ||
        M * H > kSddmmMaxNnz / 2)
        return false;
    if ((r.V != 1 && r.V != 2 && r.V != 4) || (F % r.V) != 0 || r.W < 4 || r.W > 64 || (r.W & (r.W - 1)) != 0 || 8 * (int64_t)r.W < F)
        return false;
    return !(drop && !drop->seed);
}

hipError_t ga_row_part(const int32_t* rowptr, const int32_t* colind, const float* xl, const float* xr, const float* att, const float* stats,
                       const float* out, const float* grad_out, float* delta, float* grad_xl, float* att_part, int64_t M, int64_t H,
                       int64_t F, float slope, const Gatv2AttentionLaunch& r, const EdgeDropout* drop, hipStream_t st) {
    const int leaky = slope != 1.0f ? 1 : 0;
    GESPMM_GA_SWITCH(gatv2_attention_backward_row_kernel, (, true), M * H, rowptr, colind, xl, xr, att, stats, out, grad_out, delta, grad_xl,
                     att_part, (int)M, (int)H, (int)F, slope, leaky)
}

hipError_t ga_row_plain(const int32_t* rowptr, const int32_t* colind, const float* xl, const float* xr, const float* att, const float* stats,
                        const float* out, const float* grad_out, float* delta, float* grad_xl, int64_t M, int64_t H, int64_t F, float slope,
                        const Gatv2AttentionLaunch& r, const EdgeDropout* drop, hipStream_t st) {
    const int leaky = slope != 1.0f ? 1 : 0;
    float* const none = nullptr;
    GESPMM_GA_SWITCH(gatv2_attention_backward_row_kernel, (, false), M * H, rowptr, colind, xl, xr, att, stats, out, grad_out, delta, grad_xl,
                     none, (int)M, (int)H, (int)F, slope, leaky)
}

}  // namespace

hipError_t launch_gatv2_attention(const int32_t* rowptr, const int32_t* colind, const float* xl, const float* xr, const float* att,
                                  float* out, float* stats, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope,
                                  const Gatv2AttentionLaunch& r, const EdgeDropout* drop, hipStream_t st) {
    if (!ga_launchable(M, K, H, F, nnz, r, drop)) return hipErrorInvalidValue;
    const int leaky = slope != 1.0f ? 1 : 0;
    GESPMM_GA_SWITCH(gatv2_attention_kernel, (), M * H, rowptr, colind, xl, xr, att, out, stats, (int)M, (int)H, (int)F, slope, leaky)
}

hipError_t launch_gatv2_attention_backward_row(const int32_t* rowptr, const int32_t* colind, const float* xl, const float* xr,
                                               const float* att, const float* stats, const float* out, const float* grad_out, float* delta,
                                               float* grad_xl, float* att_part, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz,
                                               float slope, const Gatv2AttentionLaunch& r, const EdgeDropout* drop, hipStream_t st) {
    if (!ga_launchable(M, K, H, F, nnz, r, drop)) return hipErrorInvalidValue;
    if (att_part) return ga_row_part(rowptr, colind, xl, xr, att, stats, out, grad_out, delta, grad_xl, att_part, M, H, F, slope, r, drop, st);
    return ga_row_plain(rowptr, colind, xl, xr, att, stats, out, grad_out, delta, grad_xl, M, H, F, slope, r, drop, st);
}

hipError_t launch_gatv2_attention_backward_col(const int32_t* colptr, const int32_t* rowind, const float* xl, const float* xr,
                                               const float* att, const float* stats, const float* delta, const float* grad_out,
                                               float* grad_xr, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope,
                                               const Gatv2AttentionLaunch& r, const EdgeDropout* drop, hipStream_t st) {
    if (!ga_launchable(M, K, H, F, nnz, r, drop)) return hipErrorInvalidValue;
    const int leaky = slope != 1.0f ? 1 : 0;
    GESPMM_GA_SWITCH(gatv2_attention_backward_col_kernel, (), K * H, colptr, rowind, xl, xr, att, stats, delta, grad_out, grad_xr, (int)K,
                     (int)H, (int)F, slope, leaky)
}

}  // namespace gespmm
