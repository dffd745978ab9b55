// dot_attention.hip — fused scaled dot-product attention over a sparsity pattern and its backward on fp32 operands (gfx950). Contract,
// geometry, pinned orders and safety rules: dot_attention.h.
//
//     s_p = scale <q[r, h, :], k[c, h, :]>      a_p = exp(s_p - m) / l      out[r, h, :] = sum_p a_p v[c, h, :]

#include "dot_attention.h"

#include "spmm_kernels.h"

namespace gespmm {

namespace {

template <int V> struct DaVec;
template <> struct DaVec<1> { using type = float; };
template <> struct DaVec<2> { using type = float __attribute__((ext_vector_type(2))); };
template <> struct DaVec<4> { using type = float __attribute__((ext_vector_type(4))); };

template <int V> __device__ __forceinline__ float da_get(const typename DaVec<V>::type& x, int i) {
    if constexpr (V == 1) return x;
    else return x[i];
}
template <int V> __device__ __forceinline__ void da_set(typename DaVec<V>::type& x, int i, float v) {
    if constexpr (V == 1) x = v;
    else x[i] = v;
}

// The seed's two words and the two kernel arguments of a dropout launch (wave-uniform).
struct DaDrop {
    uint32_t s0, s1, threshold;
    float scale;
};

// What a lane group knows about its pair.
struct DaPair {
    int pair;   // segment * H + h, clamped to the last pair for an idle group
    int seg, h;
    int lo, d;  // the segment's entries [lo, lo + d); d == 0 for an idle group
    int dmax;   // the longest segment among the wavefront's groups (wave-uniform)
    bool live;
};

template <int W>
__device__ __forceinline__ DaPair da_pair(const int32_t* __restrict__ ptr, int pair0, int g, int P, int H) {
    DaPair p;
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
__device__ __forceinline__ void da_load(const float* __restrict__ base, int l, int F, int nT, typename DaVec<V>::type (&x)[NT]) {
    using T = typename DaVec<V>::type;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        x[t] = T{};
        if (t < nT) {
            const int j = l * V + t * W * V;
            const bool in = j < F;  // (V divides F: a vector is inside the slice or past it, whole)
            const T y = *reinterpret_cast<const T*>(base + (in ? j : 0));
#pragma unroll
            for (int i = 0; i < V; ++i) da_set<V>(x[t], i, in ? da_get<V>(y, i) : 0.0f);
        }
    }
}

// The lane's chain of the pinned dot (before the butterfly).
template <int V, int NT>
__device__ __forceinline__ float da_chain(const typename DaVec<V>::type (&x)[NT], const typename DaVec<V>::type (&y)[NT], int nT) {
    float acc = 0.0f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t < nT) {
#pragma unroll
            for (int i = 0; i < V; ++i) acc = __builtin_fmaf(da_get<V>(x[t], i), da_get<V>(y[t], i), acc);
        }
    }
    return acc;
}

template <int W> __device__ __forceinline__ float da_butterfly(float x) {
#pragma unroll
    for (int m = W >> 1; m > 0; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

template <int V, int W, int NT>
__device__ __forceinline__ void da_store(float* __restrict__ base, int l, int F, int nT, const typename DaVec<V>::type (&x)[NT]) {
    using T = typename DaVec<V>::type;
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
__device__ __forceinline__ int da_index(const int32_t* __restrict__ ind, const DaPair& p, int pe) {
    return ind[pe < p.d ? p.lo + pe : (p.d > 0 ? p.lo : 0)];
}

constexpr int kDaUnroll = 2;  // entries whose gathers (both operands) are in flight per lane group

// ---- forward
template <int V, int W, bool DROP>
__device__ __forceinline__ void dot_attention_body(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                   const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                   float* __restrict__ out, float* __restrict__ stats, int M, int H, int F, float scale,
                                                   const EdgeDropout& drop) {
    constexpr int G = 64 / W;
    constexpr int NT = 8 / V;
    constexpr int UG = kDaUnroll;
    using T = typename DaVec<V>::type;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / W;
    const int l = lane % W;
    const int P = M * H;  // (M H F <= kSddmmMaxNnz: 32-bit word positions)
    const int pair0 = (blockIdx.x * kWaves + wave) * G;
    if (pair0 >= P) return;  // whole wavefront
    DaDrop dw = {};
    if constexpr (DROP) dw = {drop.seed[0], drop.seed[1], drop.threshold, drop.scale};  // wave-uniform loads
    const DaPair p = da_pair<W>(rowptr, pair0, g, P, H);
    const int nT = (F + W * V - 1) / (W * V);
    const int ld = H * F;
    const int off = p.h * F;
    T qs[NT], acc[NT];
    da_load<V, W, NT>(q + p.pair * F, l, F, nT, qs);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = T{};
    float m = 0.0f, lsum = 0.0f;
    for (int p0 = 0; p0 < p.dmax; p0 += W) {
        const int c = da_index(colind, p, p0 + l);
        const int kmax = (p.dmax - p0 < W) ? p.dmax - p0 : W;
        for (int k0 = 0; k0 < kmax; k0 += UG) {
            T kv[UG][NT], vv[UG][NT];
            int ck[UG];
#pragma unroll
            for (int u = 0; u < UG; ++u) {  // (W is a multiple of UG: k0 + u < W)
                ck[u] = __shfl(c, k0 + u, W);
                da_load<V, W, NT>(k + ck[u] * ld + off, l, F, nT, kv[u]);
                da_load<V, W, NT>(v + ck[u] * ld + off, l, F, nT, vv[u]);
            }
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                const int e = p0 + k0 + u;
                const bool valid = e < p.d;
                const float s = scale * da_butterfly<W>(da_chain<V, NT>(qs, kv[u], nT));
                const float mo = e == 0 ? s : m;  // the first entry: c = t = __expf(0) = 1, l = 1, acc = v
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
                        const float a = da_get<V>(acc[t], i);
                        const float an = __builtin_fmaf(tv, da_get<V>(vv[u][t], i), a * cc);
                        da_set<V>(acc[t], i, valid ? an : a);
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
        for (int i = 0; i < V; ++i) da_set<V>(acc[t], i, some ? da_get<V>(acc[t], i) / lsum : 0.0f);
    }
    if (p.live) {
        da_store<V, W, NT>(out + p.pair * F, l, F, nT, acc);
        if (l == 0) *reinterpret_cast<float2*>(stats + 2 * p.pair) = make_float2(m, lsum);
    }
}

// ---- backward, row pass
template <int V, int W, bool DROP>
__device__ __forceinline__ void dot_attention_backward_q_body(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                              const float* __restrict__ q, const float* __restrict__ k,
                                                              const float* __restrict__ v, const float* __restrict__ stats,
                                                              const float* __restrict__ out, const float* __restrict__ grad_out,
                                                              float* __restrict__ delta, float* __restrict__ grad_q, int M, int H, int F,
                                                              float scale, const EdgeDropout& drop) {
    constexpr int G = 64 / W;
    constexpr int NT = 8 / V;
    constexpr int UG = kDaUnroll;
    using T = typename DaVec<V>::type;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / W;
    const int l = lane % W;
    const int P = M * H;
    const int pair0 = (blockIdx.x * kWaves + wave) * G;
    if (pair0 >= P) return;  // whole wavefront
    DaDrop dw = {};
    if constexpr (DROP) dw = {drop.seed[0], drop.seed[1], drop.threshold, drop.scale};
    const DaPair p = da_pair<W>(rowptr, pair0, g, P, H);
    const int nT = (F + W * V - 1) / (W * V);
    const int ld = H * F;
    const int off = p.h * F;
    T qs[NT], gs[NT], acc[NT];
    float dl;
    {
        T os[NT];
        da_load<V, W, NT>(grad_out + p.pair * F, l, F, nT, gs);
        da_load<V, W, NT>(out + p.pair * F, l, F, nT, os);
        dl = da_butterfly<W>(da_chain<V, NT>(gs, os, nT));
    }
    da_load<V, W, NT>(q + p.pair * F, l, F, nT, qs);
    const float2 ml = *reinterpret_cast<const float2*>(stats + 2 * p.pair);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = T{};
    for (int p0 = 0; p0 < p.dmax; p0 += W) {
        const int c = da_index(colind, p, p0 + l);
        const int kmax = (p.dmax - p0 < W) ? p.dmax - p0 : W;
        for (int k0 = 0; k0 < kmax; k0 += UG) {
            T kv[UG][NT], vv[UG][NT];
            int ck[UG];
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                ck[u] = __shfl(c, k0 + u, W);
                da_load<V, W, NT>(k + ck[u] * ld + off, l, F, nT, kv[u]);
                da_load<V, W, NT>(v + ck[u] * ld + off, l, F, nT, vv[u]);
            }
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                const bool valid = p0 + k0 + u < p.d;
                const float s = scale * da_butterfly<W>(da_chain<V, NT>(qs, kv[u], nT));
                float gp = da_butterfly<W>(da_chain<V, NT>(gs, vv[u], nT));
                if constexpr (DROP)
                    gp = edge_dropout_apply(gp, edge_dropout_bits(dw.s0, dw.s1, (uint32_t)p.seg, (uint32_t)ck[u], (uint32_t)p.h), dw.threshold,
                                            dw.scale);
                const float a = __expf(s - ml.x) / ml.y;
                const float ds = a * (gp - dl);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
#pragma unroll
                    for (int i = 0; i < V; ++i) {
                        const float o = da_get<V>(acc[t], i);
                        const float n = __builtin_fmaf(ds, da_get<V>(kv[u][t], i), o);
                        da_set<V>(acc[t], i, valid ? n : o);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int i = 0; i < V; ++i) da_set<V>(acc[t], i, scale * da_get<V>(acc[t], i));
    }
    if (p.live) {
        da_store<V, W, NT>(grad_q + p.pair * F, l, F, nT, acc);
        if (l == 0) delta[p.pair] = dl;
    }
}

// ---- backward, column pass: segment = column c of the pattern, index = row r
template <int V, int W, bool DROP>
__device__ __forceinline__ void dot_attention_backward_kv_body(const int32_t* __restrict__ colptr, const int32_t* __restrict__ rowind,
                                                               const float* __restrict__ q, const float* __restrict__ k,
                                                               const float* __restrict__ v, const float* __restrict__ stats,
                                                               const float* __restrict__ delta, const float* __restrict__ grad_out,
                                                               float* __restrict__ grad_k, float* __restrict__ grad_v, int K, int H, int F,
                                                               float scale, const EdgeDropout& drop) {
    constexpr int G = 64 / W;
    constexpr int NT = 8 / V;
    constexpr int UG = kDaUnroll;
    using T = typename DaVec<V>::type;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / W;
    const int l = lane % W;
    const int P = K * H;
    const int pair0 = (blockIdx.x * kWaves + wave) * G;
    if (pair0 >= P) return;  // whole wavefront
    DaDrop dw = {};
    if constexpr (DROP) dw = {drop.seed[0], drop.seed[1], drop.threshold, drop.scale};
    const DaPair p = da_pair<W>(colptr, pair0, g, P, H);
    const int nT = (F + W * V - 1) / (W * V);
    T ks[NT], vs[NT], gk[NT], gv[NT];
    da_load<V, W, NT>(k + p.pair * F, l, F, nT, ks);
    da_load<V, W, NT>(v + p.pair * F, l, F, nT, vs);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        gk[t] = T{};
        gv[t] = T{};
    }
    for (int p0 = 0; p0 < p.dmax; p0 += W) {
        const int r = da_index(rowind, p, p0 + l);
        const int kmax = (p.dmax - p0 < W) ? p.dmax - p0 : W;
        for (int k0 = 0; k0 < kmax; k0 += UG) {
            T qv[UG][NT], ov[UG][NT];
            float2 ml[UG];
            float dl[UG];
            int rk[UG];
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                rk[u] = __shfl(r, k0 + u, W);
                const int rp = rk[u] * H + p.h;  // the pair of the entry's row
                da_load<V, W, NT>(q + rp * F, l, F, nT, qv[u]);
                da_load<V, W, NT>(grad_out + rp * F, l, F, nT, ov[u]);
                ml[u] = *reinterpret_cast<const float2*>(stats + 2 * rp);
                dl[u] = delta[rp];
            }
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                const bool valid = p0 + k0 + u < p.d;
                const float s = scale * da_butterfly<W>(da_chain<V, NT>(qv[u], ks, nT));
                float gp = da_butterfly<W>(da_chain<V, NT>(ov[u], vs, nT));
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
                        const float ok = da_get<V>(gk[t], i), ov_ = da_get<V>(gv[t], i);
                        const float nk = __builtin_fmaf(ds, da_get<V>(qv[u][t], i), ok);
                        const float nv = __builtin_fmaf(av, da_get<V>(ov[u][t], i), ov_);
                        da_set<V>(gk[t], i, valid ? nk : ok);
                        da_set<V>(gv[t], i, valid ? nv : ov_);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int i = 0; i < V; ++i) da_set<V>(gk[t], i, scale * da_get<V>(gk[t], i));
    }
    if (p.live) {
        da_store<V, W, NT>(grad_k + p.pair * F, l, F, nT, gk);
        da_store<V, W, NT>(grad_v + p.pair * F, l, F, nT, gv);
    }
}

template <int V, int W, bool DROP>
__global__ __launch_bounds__(kThreads) void dot_attention_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                                  const float* __restrict__ q, const float* __restrict__ k,
                                                                  const float* __restrict__ v, float* __restrict__ out,
                                                                  float* __restrict__ stats, int M, int H, int F, float scale,
                                                                  EdgeDropout drop) {
    dot_attention_body<V, W, DROP>(rowptr, colind, q, k, v, out, stats, M, H, F, scale, drop);
}

template <int V, int W, bool DROP>
__global__ __launch_bounds__(kThreads) void dot_attention_backward_q_kernel(const int32_t* __restrict__ rowptr,
                                                                             const int32_t* __restrict__ colind, const float* __restrict__ q,
                                                                             const float* __restrict__ k, const float* __restrict__ v,
                                                                             const float* __restrict__ stats, const float* __restrict__ out,
                                                                             const float* __restrict__ grad_out, float* __restrict__ delta,
                                                                             float* __restrict__ grad_q, int M, int H, int F, float scale,
                                                                             EdgeDropout drop) {
    dot_attention_backward_q_body<V, W, DROP>(rowptr, colind, q, k, v, stats, out, grad_out, delta, grad_q, M, H, F, scale, drop);
}

template <int V, int W, bool DROP>
__global__ __launch_bounds__(kThreads) void dot_attention_backward_kv_kernel(const int32_t* __restrict__ colptr,
                                                                              const int32_t* __restrict__ rowind, const float* __restrict__ q,
                                                                              const float* __restrict__ k, const float* __restrict__ v,
                                                                              const float* __restrict__ stats, const float* __restrict__ delta,
                                                                              const float* __restrict__ grad_out, float* __restrict__ grad_k,
                                                                              float* __restrict__ grad_v, int K, int H, int F, float scale,
                                                                              EdgeDropout drop) {
    dot_attention_backward_kv_body<V, W, DROP>(colptr, rowind, q, k, v, stats, delta, grad_out, grad_k, grad_v, K, H, F, scale, drop);
}

// blocks that cover `pairs` (segment, head) pairs with 64 / W lane groups per wavefront
inline int da_blocks(int64_t pairs, int W) {
    const int64_t per_block = (int64_t)kWaves * (64 / W);
    return (int)((pairs + per_block - 1) / per_block);
}

// One switch over (V, W, dropout) for the three kernels: KERNEL is the template's name, the rest its arguments before `drop`.
#define GESPMM_DA_CASE(KERNEL, VV, WW, PAIRS, ...)                                                                                        \
    case VV * 100 + WW:                                                                                                                   \
        if (drop)                                                                                                                         \
            hipLaunchKernelGGL((KERNEL<VV, WW, true>), dim3(da_blocks(PAIRS, WW)), dim3(kThreads), 0, st, __VA_ARGS__, *drop);            \
        else                                                                                                                              \
            hipLaunchKernelGGL((KERNEL<VV, WW, false>), dim3(da_blocks(PAIRS, WW)), dim3(kThreads), 0, st, __VA_ARGS__, EdgeDropout{});   \
        return hipGetLastError();
#define GESPMM_DA_SWITCH(KERNEL, PAIRS, ...)                     \
    switch (r.V * 100 + r.W) {                                   \
        GESPMM_DA_CASE(KERNEL, 1, 4, PAIRS, __VA_ARGS__)         \
        GESPMM_DA_CASE(KERNEL, 1, 8, PAIRS, __VA_ARGS__)         \
        GESPMM_DA_CASE(KERNEL, 1, 16, PAIRS, __VA_ARGS__)        \
        GESPMM_DA_CASE(KERNEL, 1, 32, PAIRS, __VA_ARGS__)        \
        GESPMM_DA_CASE(KERNEL, 1, 64, PAIRS, __VA_ARGS__)        \
        GESPMM_DA_CASE(KERNEL, 2, 4, PAIRS, __VA_ARGS__)         \
        GESPMM_DA_CASE(KERNEL, 2, 8, PAIRS, __VA_ARGS__)         \
        GESPMM_DA_CASE(KERNEL, 2, 16, PAIRS, __VA_ARGS__)        \
        GESPMM_DA_CASE(KERNEL, 2, 32, PAIRS, __VA_ARGS__)        \
        GESPMM_DA_CASE(KERNEL, 2, 64, PAIRS, __VA_ARGS__)        \
        GESPMM_DA_CASE(KERNEL, 4, 4, PAIRS, __VA_ARGS__)         \
        GESPMM_DA_CASE(KERNEL, 4, 8, PAIRS, __VA_ARGS__)         \
        GESPMM_DA_CASE(KERNEL, 4, 16, PAIRS, __VA_ARGS__)        \
        GESPMM_DA_CASE(KERNEL, 4, 32, PAIRS, __VA_ARGS__)        \
        GESPMM_DA_CASE(KERNEL, 4, 64, PAIRS, __VA_ARGS__)        \
    }                                                            \
    return hipErrorInvalidValue;

// Sizes the kernels' 32-bit word positions hold, and a launch shape that covers the slice with 8 floats per lane.
bool da_launchable(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, const DotAttentionLaunch& r, const EdgeDropout* drop) {
    if (nnz < 1 || M < 1 || K < 1 || H < 1 || F < 1 || F > kDotAttentionMaxF || !r.supported) return false;
    if (nnz > kSddmmMaxNnz || M > kSddmmMaxNnz / H || K > kSddmmMaxNnz / H || M * H > kSddmmMaxNnz / F || K * H > kSddmmMaxNnz / F ||
        M * H > kSddmmMaxNnz / 2)
        return false;
    if ((r.V != 1 && r.V != 2 && r.V != 4) || (F % r.V) != 0 || r.W < 4 || r.W > 64 || (r.W & (r.W - 1)) != 0 || 8 * (int64_t)r.W < F)
        return false;
    return !(drop && !drop->seed);
}

}  // namespace

hipError_t launch_dot_attention(const int32_t* rowptr, const int32_t* colind, const float* q, const float* k, const float* v, float* out,
                                float* stats, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale,
                                const DotAttentionLaunch& r, const EdgeDropout* drop, hipStream_t st) {
    if (!da_launchable(M, K, H, F, nnz, r, drop)) return hipErrorInvalidValue;
    GESPMM_DA_SWITCH(dot_attention_kernel, M * H, rowptr, colind, q, k, v, out, stats, (int)M, (int)H, (int)F, scale)
}

hipError_t launch_dot_attention_backward_q(const int32_t* rowptr, const int32_t* colind, const float* q, const float* k, const float* v,
                                           const float* stats, const float* out, const float* grad_out, float* delta, float* grad_q,
                                           int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, const DotAttentionLaunch& r,
                                           const EdgeDropout* drop, hipStream_t st) {
    if (!da_launchable(M, K, H, F, nnz, r, drop)) return hipErrorInvalidValue;
    GESPMM_DA_SWITCH(dot_attention_backward_q_kernel, M * H, rowptr, colind, q, k, v, stats, out, grad_out, delta, grad_q, (int)M, (int)H,
                     (int)F, scale)
}

hipError_t launch_dot_attention_backward_kv(const int32_t* colptr, const int32_t* rowind, const float* q, const float* k, const float* v,
                                            const float* stats, const float* delta, const float* grad_out, float* grad_k, float* grad_v,
                                            int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, const DotAttentionLaunch& r,
                                            const EdgeDropout* drop, hipStream_t st) {
    if (!da_launchable(M, K, H, F, nnz, r, drop)) return hipErrorInvalidValue;
    GESPMM_DA_SWITCH(dot_attention_backward_kv_kernel, K * H, colptr, rowind, q, k, v, stats, delta, grad_out, grad_k, grad_v, (int)K, (int)H,
                     (int)F, scale)
}

}  // namespace gespmm
