// dot_attention_x16.hip — the fused scaled dot-product attention over a sparsity pattern and its backward on 16-bit node terms (IEEE
// fp16 / bfloat16 q, k, v, out, grad_out, grad_q, grad_k, grad_v of one type; stats, delta and scale stay fp32; gfx950). Contract,
// geometry and the bit property: dot_attention_x16.h; pinned orders and safety rules: dot_attention.h.
//
//     s_p = scale <widen(q[r, h, :]), widen(k[c, h, :])>      a_p = exp(s_p - m) / l      out[r, h, :] = narrow(sum_p a_p widen(v[c, h, :]))
//
// The three kernels of dot_attention.hip with a lane's vector counted in ELEMENTS: V elements of a 16-bit operand are one uint2 / one
// dword / one ushort load for V = 4 / 2 / 1. The segment's own slices are widened once into registers; a GATHERED vector stays packed
// until the entry is used. Every element is widened exactly (widen_x16), every 16-bit result is rounded once at its store (narrow_x16).
// The arithmetic in between is the fp32 kernels', expression for expression: no packed-fp16 arithmetic, no dot2.

#include "dot_attention_x16.h"

#include "spmm_device.h"
#include "spmm_kernels.h"

namespace gespmm {

namespace {

// V 16-bit elements as (V + 1) / 2 words, the lower-addressed element of a word in its low half (V = 1: the low half alone).
template <int V> struct Da16Vec { static constexpr int n = (V + 1) / 2; uint32_t w[n]; };

template <int V> __device__ __forceinline__ Da16Vec<V> da16_load_vec(const uint16_t* __restrict__ p) {
    Da16Vec<V> r;
    if constexpr (V == 1) {
        r.w[0] = *p;
    } else if constexpr (V == 2) {
        r.w[0] = *reinterpret_cast<const uint32_t*>(p);
    } else {
        const uint2 t = *reinterpret_cast<const uint2*>(p);
        r.w[0] = t.x, r.w[1] = t.y;
    }
    return r;
}

// element i of the vector, widened exactly
template <int DT, int V> __device__ __forceinline__ float da16_get(const Da16Vec<V>& r, int i) {
    float lo, hi;
    widen_x16<DT>(__uint_as_float(r.w[i >> 1]), lo, hi);
    return (i & 1) ? hi : lo;
}

// The seed's two words and the two kernel arguments of a dropout launch (wave-uniform).
struct Da16Drop {
    uint32_t s0, s1, threshold;
    float scale;
};

// What a lane group knows about its pair (DaPair of dot_attention.hip).
struct Da16Pair {
    int pair;   // segment * H + h, clamped to the last pair for an idle group
    int seg, h;
    int lo, d;  // the segment's entries [lo, lo + d); d == 0 for an idle group
    int dmax;   // the longest segment among the wavefront's groups (wave-uniform)
    bool live;
};

__device__ __forceinline__ Da16Pair da16_pair(const int32_t* __restrict__ ptr, int pair0, int g, int P, int H) {
    Da16Pair p;
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

// The lane's NT packed vectors of the 16-bit head slice that starts at `base`: a vector past the slice is clamped to the slice's first
// element and replaced by zero words (+0 in either type). nT = ceil(F / (W V)) is wave-uniform.
template <int V, int W, int NT>
__device__ __forceinline__ void da16_load(const uint16_t* __restrict__ base, int l, int F, int nT, Da16Vec<V> (&x)[NT]) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int k = 0; k < Da16Vec<V>::n; ++k) x[t].w[k] = 0u;
        if (t < nT) {
            const int j = l * V + t * W * V;
            const bool in = j < F;  // (V divides F: a vector is inside the slice or past it, whole)
            const Da16Vec<V> y = da16_load_vec<V>(base + (in ? j : 0));
#pragma unroll
            for (int k = 0; k < Da16Vec<V>::n; ++k) x[t].w[k] = in ? y.w[k] : 0u;
        }
    }
}

// ... widened into the lane's 8 floats: element i of vector t is f[t V + i]
template <int DT, int V, int W, int NT>
__device__ __forceinline__ void da16_load_wide(const uint16_t* __restrict__ base, int l, int F, int nT, float (&f)[8]) {
    Da16Vec<V> x[NT];
    da16_load<V, W, NT>(base, l, F, nT, x);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int i = 0; i < V; ++i) f[t * V + i] = da16_get<DT, V>(x[t], i);
    }
}

// The lane's chain of the pinned dot (before the butterfly): x the lane's floats, y a packed gathered slice. fmaf(a, b, acc) commutes
// in a and b: which of the two factors is the held one leaves no trace.
template <int DT, int V, int NT>
__device__ __forceinline__ float da16_chain(const float (&x)[8], const Da16Vec<V> (&y)[NT], int nT) {
    float acc = 0.0f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t < nT) {
#pragma unroll
            for (int i = 0; i < V; ++i) acc = __builtin_fmaf(x[t * V + i], da16_get<DT, V>(y[t], i), acc);
        }
    }
    return acc;
}

// ... with both factors in floats (delta = dot(grad_out, out))
template <int V, int NT> __device__ __forceinline__ float da16_chain_wide(const float (&x)[8], const float (&y)[8], int nT) {
    float acc = 0.0f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t < nT) {
#pragma unroll
            for (int i = 0; i < V; ++i) acc = __builtin_fmaf(x[t * V + i], y[t * V + i], acc);
        }
    }
    return acc;
}

// x, with its fp32 rounding made a fact: `zero` is a zero the compiler cannot see, added to x's bits — the sign bit of a LOADED segment
// start (the sign of a size is no secret to it inside the store's predicate j < F, where it folded the add away). Without it
// the fp16 store of fl32(scale * chain) is compiled to ONE multiply that rounds the exact product straight to fp16 (v_fma_mixlo_f16):
// a second rounding skipped, and a word that differs from the fp32 entry point's, narrowed, wherever fl32 lands on an fp16 tie.
__device__ __forceinline__ float da16_fl32(float x, uint32_t zero) { return __uint_as_float(__float_as_uint(x) + zero); }

template <int W> __device__ __forceinline__ float da16_butterfly(float x) {
#pragma unroll
    for (int m = W >> 1; m > 0; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// The lane's 8 sums, each rounded ONCE to nearest even, as packed vectors of 2 V bytes.
template <int DT, int V, int W, int NT>
__device__ __forceinline__ void da16_store(uint16_t* __restrict__ base, int l, int F, int nT, const float (&f)[8]) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t < nT) {
            const int j = l * V + t * W * V;
            if (j < F) {
                if constexpr (V == 1) {
                    base[j] = (uint16_t)narrow_x16<DT>(f[t]);
                } else if constexpr (V == 2) {
                    *reinterpret_cast<uint32_t*>(base + j) = narrow_x16<DT>(f[2 * t]) | (narrow_x16<DT>(f[2 * t + 1]) << 16);
                } else {
                    *reinterpret_cast<uint2*>(base + j) = make_uint2(narrow_x16<DT>(f[4 * t]) | (narrow_x16<DT>(f[4 * t + 1]) << 16),
                                                                     narrow_x16<DT>(f[4 * t + 2]) | (narrow_x16<DT>(f[4 * t + 3]) << 16));
                }
            }
        }
    }
}

// W indices of the group's segment, one per lane: a lane past its segment re-reads the segment's first entry (entry 0 where the segment
// is empty: nnz >= 1); what is gathered through it is dropped by a select.
__device__ __forceinline__ int da16_index(const int32_t* __restrict__ ind, const Da16Pair& p, int pe) {
    return ind[pe < p.d ? p.lo + pe : (p.d > 0 ? p.lo : 0)];
}

// Entries whose gathers (both operands) are in flight per lane group: kDaUnroll of dot_attention.hip, carried over to 16-bit rows, not
// measured on them.
constexpr int kDa16Unroll = 2;

// ---- forward
template <int DT, int V, int W, bool DROP>
__global__ __launch_bounds__(kThreads) void dot_attention_x16_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                                      const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                                                                      const uint16_t* __restrict__ v, uint16_t* __restrict__ out,
                                                                      float* __restrict__ stats, int M, int H, int F, float scale,
                                                                      EdgeDropout drop) {
    constexpr int G = 64 / W;
    constexpr int NT = 8 / V;
    constexpr int UG = kDa16Unroll;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / W;
    const int l = lane % W;
    const int P = M * H;  // (M H F <= kSddmmMaxNnz: 32-bit element positions)
    const int pair0 = (blockIdx.x * kWaves + wave) * G;
    if (pair0 >= P) return;  // whole wavefront
    Da16Drop dw = {};
    if constexpr (DROP) dw = {drop.seed[0], drop.seed[1], drop.threshold, drop.scale};  // wave-uniform loads
    const Da16Pair p = da16_pair(rowptr, pair0, g, P, H);
    const int nT = (F + W * V - 1) / (W * V);
    const int ld = H * F;
    const int off = p.h * F;
    float qs[8], acc[8];
    da16_load_wide<DT, V, W, NT>(q + p.pair * F, l, F, nT, qs);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
    float m = 0.0f, lsum = 0.0f;
    for (int p0 = 0; p0 < p.dmax; p0 += W) {
        const int c = da16_index(colind, p, p0 + l);
        const int kmax = (p.dmax - p0 < W) ? p.dmax - p0 : W;
        for (int k0 = 0; k0 < kmax; k0 += UG) {
            Da16Vec<V> kv[UG][NT], vv[UG][NT];
            int ck[UG];
#pragma unroll
            for (int u = 0; u < UG; ++u) {  // (W is a multiple of UG: k0 + u < W)
                ck[u] = __shfl(c, k0 + u, W);
                da16_load<V, W, NT>(k + ck[u] * ld + off, l, F, nT, kv[u]);
                da16_load<V, W, NT>(v + ck[u] * ld + off, l, F, nT, vv[u]);
            }
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                const int e = p0 + k0 + u;
                const bool valid = e < p.d;
                const float s = scale * da16_butterfly<W>(da16_chain<DT, V, NT>(qs, kv[u], nT));
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
                        const float a = acc[t * V + i];
                        const float an = __builtin_fmaf(tv, da16_get<DT, V>(vv[u][t], i), a * cc);
                        acc[t * V + i] = valid ? an : a;
                    }
                }
                m = valid ? mn : m;
                lsum = valid ? ln : lsum;
            }
        }
    }
    const bool some = p.d > 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = some ? acc[j] / lsum : 0.0f;
    if (p.live) {
        da16_store<DT, V, W, NT>(out + p.pair * F, l, F, nT, acc);  // ONE rounding per element
        if (l == 0) *reinterpret_cast<float2*>(stats + 2 * p.pair) = make_float2(m, lsum);
    }
}

// ---- backward, row pass
template <int DT, int V, int W, bool DROP>
__global__ __launch_bounds__(kThreads) void dot_attention_backward_q_x16_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind, const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, const float* __restrict__ stats, const uint16_t* __restrict__ out, const uint16_t* __restrict__ grad_out,
    float* __restrict__ delta, uint16_t* __restrict__ grad_q, int M, int H, int F, float scale, EdgeDropout drop) {
    constexpr int G = 64 / W;
    constexpr int NT = 8 / V;
    constexpr int UG = kDa16Unroll;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / W;
    const int l = lane % W;
    const int P = M * H;
    const int pair0 = (blockIdx.x * kWaves + wave) * G;
    if (pair0 >= P) return;  // whole wavefront
    Da16Drop dw = {};
    if constexpr (DROP) dw = {drop.seed[0], drop.seed[1], drop.threshold, drop.scale};
    const Da16Pair p = da16_pair(rowptr, pair0, g, P, H);
    const int nT = (F + W * V - 1) / (W * V);
    const int ld = H * F;
    const int off = p.h * F;
    float qs[8], gs[8], acc[8];
    float dl;
    {
        float os[8];  // the STORED out: what the forward rounded
        da16_load_wide<DT, V, W, NT>(grad_out + p.pair * F, l, F, nT, gs);
        da16_load_wide<DT, V, W, NT>(out + p.pair * F, l, F, nT, os);
        dl = da16_butterfly<W>(da16_chain_wide<V, NT>(gs, os, nT));
    }
    da16_load_wide<DT, V, W, NT>(q + p.pair * F, l, F, nT, qs);
    const float2 ml = *reinterpret_cast<const float2*>(stats + 2 * p.pair);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
    for (int p0 = 0; p0 < p.dmax; p0 += W) {
        const int c = da16_index(colind, p, p0 + l);
        const int kmax = (p.dmax - p0 < W) ? p.dmax - p0 : W;
        for (int k0 = 0; k0 < kmax; k0 += UG) {
            Da16Vec<V> kv[UG][NT], vv[UG][NT];
            int ck[UG];
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                ck[u] = __shfl(c, k0 + u, W);
                da16_load<V, W, NT>(k + ck[u] * ld + off, l, F, nT, kv[u]);
                da16_load<V, W, NT>(v + ck[u] * ld + off, l, F, nT, vv[u]);
            }
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                const bool valid = p0 + k0 + u < p.d;
                const float s = scale * da16_butterfly<W>(da16_chain<DT, V, NT>(qs, kv[u], nT));
                float gp = da16_butterfly<W>(da16_chain<DT, V, NT>(gs, vv[u], nT));
                if constexpr (DROP)
                    gp = edge_dropout_apply(gp, edge_dropout_bits(dw.s0, dw.s1, (uint32_t)p.seg, (uint32_t)ck[u], (uint32_t)p.h), dw.threshold,
                                            dw.scale);
                const float a = __expf(s - ml.x) / ml.y;
                const float ds = a * (gp - dl);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
#pragma unroll
                    for (int i = 0; i < V; ++i) {
                        const float o = acc[t * V + i];
                        const float n = __builtin_fmaf(ds, da16_get<DT, V>(kv[u][t], i), o);
                        acc[t * V + i] = valid ? n : o;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = da16_fl32(scale * acc[j], (uint32_t)p.lo >> 31);  // fl32(scale * chain); the store rounds it once
    if (p.live) {
        da16_store<DT, V, W, NT>(grad_q + p.pair * F, l, F, nT, acc);
        if (l == 0) delta[p.pair] = dl;
    }
}

// ---- backward, column pass: segment = column c of the pattern, index = row r
template <int DT, int V, int W, bool DROP>
__global__ __launch_bounds__(kThreads) void dot_attention_backward_kv_x16_kernel(
    const int32_t* __restrict__ colptr, const int32_t* __restrict__ rowind, const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, const float* __restrict__ stats, const float* __restrict__ delta, const uint16_t* __restrict__ grad_out,
    uint16_t* __restrict__ grad_k, uint16_t* __restrict__ grad_v, int K, int H, int F, float scale, EdgeDropout drop) {
    constexpr int G = 64 / W;
    constexpr int NT = 8 / V;
    constexpr int UG = kDa16Unroll;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / W;
    const int l = lane % W;
    const int P = K * H;
    const int pair0 = (blockIdx.x * kWaves + wave) * G;
    if (pair0 >= P) return;  // whole wavefront
    Da16Drop dw = {};
    if constexpr (DROP) dw = {drop.seed[0], drop.seed[1], drop.threshold, drop.scale};
    const Da16Pair p = da16_pair(colptr, pair0, g, P, H);
    const int nT = (F + W * V - 1) / (W * V);
    float ks[8], vs[8], gk[8], gv[8];
    da16_load_wide<DT, V, W, NT>(k + p.pair * F, l, F, nT, ks);
    da16_load_wide<DT, V, W, NT>(v + p.pair * F, l, F, nT, vs);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        gk[j] = 0.0f;
        gv[j] = 0.0f;
    }
    for (int p0 = 0; p0 < p.dmax; p0 += W) {
        const int r = da16_index(rowind, p, p0 + l);
        const int kmax = (p.dmax - p0 < W) ? p.dmax - p0 : W;
        for (int k0 = 0; k0 < kmax; k0 += UG) {
            Da16Vec<V> qv[UG][NT], ov[UG][NT];
            float2 ml[UG];
            float dl[UG];
            int rk[UG];
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                rk[u] = __shfl(r, k0 + u, W);
                const int rp = rk[u] * H + p.h;  // the pair of the entry's row
                da16_load<V, W, NT>(q + rp * F, l, F, nT, qv[u]);
                da16_load<V, W, NT>(grad_out + rp * F, l, F, nT, ov[u]);
                ml[u] = *reinterpret_cast<const float2*>(stats + 2 * rp);
                dl[u] = delta[rp];
            }
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                const bool valid = p0 + k0 + u < p.d;
                const float s = scale * da16_butterfly<W>(da16_chain<DT, V, NT>(ks, qv[u], nT));
                float gp = da16_butterfly<W>(da16_chain<DT, V, NT>(vs, ov[u], nT));
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
                        const int j = t * V + i;
                        const float ok = gk[j], ov_ = gv[j];
                        const float nk = __builtin_fmaf(ds, da16_get<DT, V>(qv[u][t], i), ok);
                        const float nv = __builtin_fmaf(av, da16_get<DT, V>(ov[u][t], i), ov_);
                        gk[j] = valid ? nk : ok;
                        gv[j] = valid ? nv : ov_;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) gk[j] = da16_fl32(scale * gk[j], (uint32_t)p.lo >> 31);  // fl32(scale * chain); the store rounds it once
    if (p.live) {
        da16_store<DT, V, W, NT>(grad_k + p.pair * F, l, F, nT, gk);
        da16_store<DT, V, W, NT>(grad_v + p.pair * F, l, F, nT, gv);
    }
}

// blocks that cover `pairs` (segment, head) pairs with 64 / W lane groups per wavefront
inline int da16_blocks(int64_t pairs, int W) {
    const int64_t per_block = (int64_t)kWaves * (64 / W);
    return (int)((pairs + per_block - 1) / per_block);
}

// One switch over (V, W, dropout) for the three kernels (GESPMM_DA_SWITCH of dot_attention.hip with the type in front): KERNEL is the
// template's name, the rest its arguments before `drop`.
#define GESPMM_DA16_CASE(KERNEL, VV, WW, PAIRS, ...)                                                                                          \
    case VV * 100 + WW:                                                                                                                       \
        if (drop)                                                                                                                             \
            hipLaunchKernelGGL((KERNEL<DT, VV, WW, true>), dim3(da16_blocks(PAIRS, WW)), dim3(kThreads), 0, st, __VA_ARGS__, *drop);          \
        else                                                                                                                                  \
            hipLaunchKernelGGL((KERNEL<DT, VV, WW, false>), dim3(da16_blocks(PAIRS, WW)), dim3(kThreads), 0, st, __VA_ARGS__, EdgeDropout{}); \
        return hipGetLastError();
#define GESPMM_DA16_SWITCH(KERNEL, PAIRS, ...)                     \
    switch (r.V * 100 + r.W) {                                     \
        GESPMM_DA16_CASE(KERNEL, 1, 4, PAIRS, __VA_ARGS__)         \
        GESPMM_DA16_CASE(KERNEL, 1, 8, PAIRS, __VA_ARGS__)         \
        GESPMM_DA16_CASE(KERNEL, 1, 16, PAIRS, __VA_ARGS__)        \
        GESPMM_DA16_CASE(KERNEL, 1, 32, PAIRS, __VA_ARGS__)        \
        GESPMM_DA16_CASE(KERNEL, 1, 64, PAIRS, __VA_ARGS__)        \
        GESPMM_DA16_CASE(KERNEL, 2, 4, PAIRS, __VA_ARGS__)         \
        GESPMM_DA16_CASE(KERNEL, 2, 8, PAIRS, __VA_ARGS__)         \
        GESPMM_DA16_CASE(KERNEL, 2, 16, PAIRS, __VA_ARGS__)        \
        GESPMM_DA16_CASE(KERNEL, 2, 32, PAIRS, __VA_ARGS__)        \
        GESPMM_DA16_CASE(KERNEL, 2, 64, PAIRS, __VA_ARGS__)        \
        GESPMM_DA16_CASE(KERNEL, 4, 4, PAIRS, __VA_ARGS__)         \
        GESPMM_DA16_CASE(KERNEL, 4, 8, PAIRS, __VA_ARGS__)         \
        GESPMM_DA16_CASE(KERNEL, 4, 16, PAIRS, __VA_ARGS__)        \
        GESPMM_DA16_CASE(KERNEL, 4, 32, PAIRS, __VA_ARGS__)        \
        GESPMM_DA16_CASE(KERNEL, 4, 64, PAIRS, __VA_ARGS__)        \
    }                                                              \
    return hipErrorInvalidValue;

// Sizes the kernels' 32-bit element positions hold, and a launch shape that covers the slice with 8 elements per lane.
bool da16_launchable(int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, const DotAttentionLaunch& r,
                     const EdgeDropout* drop) {
    if (dtype != kX16F16 && dtype != kX16Bf16) return false;
    if (nnz < 1 || M < 1 || K < 1 || H < 1 || F < 1 || F > kDotAttentionMaxF || !r.supported) return false;
    if (nnz > kSddmmMaxNnz || M > kSddmmMaxNnz / H || K > kSddmmMaxNnz / H || M * H > kSddmmMaxNnz / F || K * H > kSddmmMaxNnz / F ||
        M * H > kSddmmMaxNnz / 2)
        return false;
    if ((r.V != 1 && r.V != 2 && r.V != 4) || (F % r.V) != 0 || r.W < 4 || r.W > 64 || (r.W & (r.W - 1)) != 0 || 8 * (int64_t)r.W < F)
        return false;
    return !(drop && !drop->seed);
}

template <int DT>
hipError_t da16_forward(const int32_t* rowptr, const int32_t* colind, const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* out,
                        float* stats, int64_t M, int64_t H, int64_t F, float scale, const DotAttentionLaunch& r, const EdgeDropout* drop,
                        hipStream_t st) {
    GESPMM_DA16_SWITCH(dot_attention_x16_kernel, M * H, rowptr, colind, q, k, v, out, stats, (int)M, (int)H, (int)F, scale)
}

template <int DT>
hipError_t da16_backward_q(const int32_t* rowptr, const int32_t* colind, const uint16_t* q, const uint16_t* k, const uint16_t* v,
                           const float* stats, const uint16_t* out, const uint16_t* grad_out, float* delta, uint16_t* grad_q, int64_t M,
                           int64_t H, int64_t F, float scale, const DotAttentionLaunch& r, const EdgeDropout* drop, hipStream_t st) {
    GESPMM_DA16_SWITCH(dot_attention_backward_q_x16_kernel, M * H, rowptr, colind, q, k, v, stats, out, grad_out, delta, grad_q, (int)M,
                       (int)H, (int)F, scale)
}

template <int DT>
hipError_t da16_backward_kv(const int32_t* colptr, const int32_t* rowind, const uint16_t* q, const uint16_t* k, const uint16_t* v,
                            const float* stats, const float* delta, const uint16_t* grad_out, uint16_t* grad_k, uint16_t* grad_v, int64_t K,
                            int64_t H, int64_t F, float scale, const DotAttentionLaunch& r, const EdgeDropout* drop, hipStream_t st) {
    GESPMM_DA16_SWITCH(dot_attention_backward_kv_x16_kernel, K * H, colptr, rowind, q, k, v, stats, delta, grad_out, grad_k, grad_v, (int)K,
                       (int)H, (int)F, scale)
}

inline const uint16_t* u16(const void* p) { return static_cast<const uint16_t*>(p); }
inline uint16_t* u16(void* p) { return static_cast<uint16_t*>(p); }

}  // namespace

hipError_t launch_dot_attention_x16(const int32_t* rowptr, const int32_t* colind, const void* q, const void* k, const void* v, void* out,
                                    float* stats, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale,
                                    const DotAttentionLaunch& r, const EdgeDropout* drop, hipStream_t st) {
    if (!da16_launchable(dtype, M, K, H, F, nnz, r, drop)) return hipErrorInvalidValue;
    if (dtype == kX16F16) return da16_forward<kX16F16>(rowptr, colind, u16(q), u16(k), u16(v), u16(out), stats, M, H, F, scale, r, drop, st);
    return da16_forward<kX16Bf16>(rowptr, colind, u16(q), u16(k), u16(v), u16(out), stats, M, H, F, scale, r, drop, st);
}

hipError_t launch_dot_attention_backward_q_x16(const int32_t* rowptr, const int32_t* colind, const void* q, const void* k, const void* v,
                                               const float* stats, const void* out, const void* grad_out, float* delta, void* grad_q,
                                               int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale,
                                               const DotAttentionLaunch& r, const EdgeDropout* drop, hipStream_t st) {
    if (!da16_launchable(dtype, M, K, H, F, nnz, r, drop)) return hipErrorInvalidValue;
    if (dtype == kX16F16)
        return da16_backward_q<kX16F16>(rowptr, colind, u16(q), u16(k), u16(v), stats, u16(out), u16(grad_out), delta, u16(grad_q), M, H, F,
                                        scale, r, drop, st);
    return da16_backward_q<kX16Bf16>(rowptr, colind, u16(q), u16(k), u16(v), stats, u16(out), u16(grad_out), delta, u16(grad_q), M, H, F, scale,
                                     r, drop, st);
}

hipError_t launch_dot_attention_backward_kv_x16(const int32_t* colptr, const int32_t* rowind, const void* q, const void* k, const void* v,
                                                const float* stats, const float* delta, const void* grad_out, void* grad_k, void* grad_v,
                                                int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale,
                                                const DotAttentionLaunch& r, const EdgeDropout* drop, hipStream_t st) {
    if (!da16_launchable(dtype, M, K, H, F, nnz, r, drop)) return hipErrorInvalidValue;
    if (dtype == kX16F16)
        return da16_backward_kv<kX16F16>(colptr, rowind, u16(q), u16(k), u16(v), stats, delta, u16(grad_out), u16(grad_k), u16(grad_v), K, H, F,
                                         scale, r, drop, st);
    return da16_backward_kv<kX16Bf16>(colptr, rowind, u16(q), u16(k), u16(v), stats, delta, u16(grad_out), u16(grad_k), u16(grad_v), K, H, F,
                                      scale, r, drop, st);
}

}  // namespace gespmm
