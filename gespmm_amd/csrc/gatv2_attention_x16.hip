// gatv2_attention_x16.hip — the fused GATv2 attention over a sparsity pattern and its backward on 16-bit node terms (IEEE fp16 /
// bfloat16 xl, xr, out, grad_out, grad_xl, grad_xr of one type; att, stats, delta and att_part stay fp32; gfx950). Contract, geometry
// and the bit property: gatv2_attention_x16.h; pinned orders and safety rules: gatv2_attention.h.
//
//     s_p = sum_f att[h, f] leaky(fl32(widen(xl[r, h, f]) + widen(xr[c, h, f])))      a_p = exp(s_p - m) / l
//     out[r, h, :] = narrow(sum_p a_p widen(xr[c, h, :]))
//
// The three kernels of gatv2_attention.hip with a lane's vector counted in ELEMENTS: V elements of a 16-bit operand are one uint2 / one
// dword / one ushort load for V = 4 / 2 / 1, the V floats of att at the same element positions one float4 / float2 / float load. The
// segment's own slices are widened once into registers; a GATHERED vector stays packed until the entry is used. Every element is widened
// exactly (widen_x16), every 16-bit result is rounded once at its store (narrow_x16). The arithmetic in between is the fp32 kernels',
// expression for expression: no packed-fp16 arithmetic, no dot2.

#include "gatv2_attention_x16.h"

#include "spmm_device.h"
#include "spmm_kernels.h"

namespace gespmm {

namespace {

// V 16-bit elements as (V + 1) / 2 words, the lower-addressed element of a word in its low half (V = 1: the low half alone).
template <int V> struct Ga16Vec { static constexpr int n = (V + 1) / 2; uint32_t w[n]; };

template <int V> __device__ __forceinline__ Ga16Vec<V> ga16_load_vec(const uint16_t* __restrict__ p) {
    Ga16Vec<V> r;
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
template <int DT, int V> __device__ __forceinline__ float ga16_get(const Ga16Vec<V>& r, int i) {
    float lo, hi;
    widen_x16<DT>(__uint_as_float(r.w[i >> 1]), lo, hi);
    return (i & 1) ? hi : lo;
}

// The seed's two words and the two kernel arguments of a dropout launch (wave-uniform).
struct Ga16Drop {
    uint32_t s0, s1, threshold;
    float scale;
};

// What a lane group knows about its pair (GaPair of gatv2_attention.hip).
struct Ga16Pair {
    int pair;   // segment * H + h, clamped to the last pair for an idle group
    int seg, h;
    int lo, d;  // the segment's entries [lo, lo + d); d == 0 for an idle group
    int dmax;   // the longest segment among the wavefront's groups (wave-uniform)
    bool live;
};

__device__ __forceinline__ Ga16Pair ga16_pair(const int32_t* __restrict__ ptr, int pair0, int g, int P, int H) {
    Ga16Pair p;
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
__device__ __forceinline__ void ga16_load(const uint16_t* __restrict__ base, int l, int F, int nT, Ga16Vec<V> (&x)[NT]) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int k = 0; k < Ga16Vec<V>::n; ++k) x[t].w[k] = 0u;
        if (t < nT) {
            const int j = l * V + t * W * V;
            const bool in = j < F;  // (V divides F: a vector is inside the slice or past it, whole)
            const Ga16Vec<V> y = ga16_load_vec<V>(base + (in ? j : 0));
#pragma unroll
            for (int k = 0; k < Ga16Vec<V>::n; ++k) x[t].w[k] = in ? y.w[k] : 0u;
        }
    }
}

// ... widened into the lane's 8 floats: element i of vector t is f[t V + i]
template <int DT, int V, int W, int NT>
__device__ __forceinline__ void ga16_load_wide(const uint16_t* __restrict__ base, int l, int F, int nT, float (&f)[8]) {
    Ga16Vec<V> x[NT];
    ga16_load<V, W, NT>(base, l, F, nT, x);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int i = 0; i < V; ++i) f[t * V + i] = ga16_get<DT, V>(x[t], i);
    }
}

// The lane's floats of an fp32 slice (att) at the element positions of the 16-bit vectors: one load of 4 V bytes per vector.
template <int V, int W, int NT>
__device__ __forceinline__ void ga16_load_f32(const float* __restrict__ base, int l, int F, int nT, float (&f)[8]) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int i = 0; i < V; ++i) f[t * V + i] = 0.0f;
        if (t < nT) {
            const int j = l * V + t * W * V;
            const bool in = j < F;
            const float* q = base + (in ? j : 0);
            float y[V];
            if constexpr (V == 1) {
                y[0] = *q;
            } else if constexpr (V == 2) {
                const float2 v = *reinterpret_cast<const float2*>(q);
                y[0] = v.x, y[1] = v.y;
            } else {
                const float4 v = *reinterpret_cast<const float4*>(q);
                y[0] = v.x, y[1] = v.y, y[2] = v.z, y[3] = v.w;
            }
#pragma unroll
            for (int i = 0; i < V; ++i) f[t * V + i] = in ? y[i] : 0.0f;
        }
    }
}

// leaky(t) = t >= 0 ? t : slope * t. `leaky` is false for slope == 1: no multiply. (The expression of gatv2_attention.hip.)
__device__ __forceinline__ float ga16_leaky(float t, float slope, bool leaky) { return (leaky && !(t >= 0.0f)) ? slope * t : t; }

// The lane's chain of the pinned dot (before the butterfly): x the lane's floats, y a packed gathered slice.
template <int DT, int V, int NT>
__device__ __forceinline__ float ga16_chain(const float (&x)[8], const Ga16Vec<V> (&y)[NT], int nT) {
    float acc = 0.0f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t < nT) {
#pragma unroll
            for (int i = 0; i < V; ++i) acc = __builtin_fmaf(x[t * V + i], ga16_get<DT, V>(y[t], i), acc);
        }
    }
    return acc;
}

// ... with both factors in floats (delta = dot(grad_out, out))
template <int V, int NT> __device__ __forceinline__ float ga16_chain_wide(const float (&x)[8], const float (&y)[8], int nT) {
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

// The lane's chain of the score: fmaf(att_j, leaky(fl(x_j + y_j)), acc), x the lane's floats and y the packed gathered slice. (The fp32
// add commutes: the column pass, whose gathered slice is xl, computes the same bits.) A lane past the slice holds zeros: fmaf(0, 0, acc).
template <int DT, int V, int NT>
__device__ __forceinline__ float ga16_score_chain(const float (&a)[8], const float (&x)[8], const Ga16Vec<V> (&y)[NT], int nT, float slope,
                                                  bool leaky) {
    float acc = 0.0f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t < nT) {
#pragma unroll
            for (int i = 0; i < V; ++i)
                acc = __builtin_fmaf(a[t * V + i], ga16_leaky(x[t * V + i] + ga16_get<DT, V>(y[t], i), slope, leaky), acc);
        }
    }
    return acc;
}

template <int W> __device__ __forceinline__ float ga16_butterfly(float x) {
#pragma unroll
    for (int m = W >> 1; m > 0; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// The lane's 8 sums, each rounded ONCE to nearest even, as packed vectors of 2 V bytes.
template <int DT, int V, int W, int NT>
__device__ __forceinline__ void ga16_store(uint16_t* __restrict__ base, int l, int F, int nT, const float (&f)[8]) {
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

template <int V, int W, int NT> __device__ __forceinline__ void ga16_store_f32(float* __restrict__ base, int l, int F, int nT, const float (&f)[8]) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t < nT) {
            const int j = l * V + t * W * V;
            if (j < F) {
                if constexpr (V == 1) base[j] = f[t];
                else if constexpr (V == 2) *reinterpret_cast<float2*>(base + j) = make_float2(f[2 * t], f[2 * t + 1]);
                else *reinterpret_cast<float4*>(base + j) = make_float4(f[4 * t], f[4 * t + 1], f[4 * t + 2], f[4 * t + 3]);
            }
        }
    }
}

// W indices of the group's segment, one per lane: a lane past its segment re-reads the segment's first entry (entry 0 where the segment
// is empty: nnz >= 1); what is gathered through it is dropped by a select.
__device__ __forceinline__ int ga16_index(const int32_t* __restrict__ ind, const Ga16Pair& p, int pe) {
    return ind[pe < p.d ? p.lo + pe : (p.d > 0 ? p.lo : 0)];
}

// Entries in flight per lane group: the depths of gatv2_attention.hip, carried over to 16-bit rows, not measured on them.
constexpr int kGa16UnrollRow = 4;  // ONE gathered row per entry: forward and row pass (W is a multiple)
constexpr int kGa16UnrollCol = 2;  // TWO gathered rows and three words per entry: column pass

// ---- forward
template <int DT, int V, int W, bool DROP>
__global__ __launch_bounds__(kThreads) void gatv2_attention_x16_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                                        const uint16_t* __restrict__ xl, const uint16_t* __restrict__ xr,
                                                                        const float* __restrict__ att, uint16_t* __restrict__ out,
                                                                        float* __restrict__ stats, int M, int H, int F, float slope,
                                                                        int leaky_i, EdgeDropout drop) {
    constexpr int G = 64 / W;
    constexpr int NT = 8 / V;
    constexpr int UG = kGa16UnrollRow;
    const bool leaky = leaky_i != 0;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / W;
    const int l = lane % W;
    const int P = M * H;  // (M H F <= kSddmmMaxNnz: 32-bit element positions)
    const int pair0 = (blockIdx.x * kWaves + wave) * G;
    if (pair0 >= P) return;  // whole wavefront
    Ga16Drop dw = {};
    if constexpr (DROP) dw = {drop.seed[0], drop.seed[1], drop.threshold, drop.scale};  // wave-uniform loads
    const Ga16Pair p = ga16_pair(rowptr, pair0, g, P, H);
    const int nT = (F + W * V - 1) / (W * V);
    const int ld = H * F;
    const int off = p.h * F;
    float xs[8], as[8], acc[8];
    ga16_load_wide<DT, V, W, NT>(xl + p.pair * F, l, F, nT, xs);
    ga16_load_f32<V, W, NT>(att + off, l, F, nT, as);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
    float m = 0.0f, lsum = 0.0f;
    for (int p0 = 0; p0 < p.dmax; p0 += W) {
        const int c = ga16_index(colind, p, p0 + l);
        const int kmax = (p.dmax - p0 < W) ? p.dmax - p0 : W;
        for (int k0 = 0; k0 < kmax; k0 += UG) {
            Ga16Vec<V> xv[UG][NT];
            int ck[UG];
#pragma unroll
            for (int u = 0; u < UG; ++u) {  // (W is a multiple of UG: k0 + u < W)
                ck[u] = __shfl(c, k0 + u, W);
                ga16_load<V, W, NT>(xr + ck[u] * ld + off, l, F, nT, xv[u]);
            }
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                const int e = p0 + k0 + u;
                const bool valid = e < p.d;
                const float s = ga16_butterfly<W>(ga16_score_chain<DT, V, NT>(as, xs, xv[u], nT, slope, leaky));
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
                        const float a = acc[t * V + i];
                        const float an = __builtin_fmaf(tv, ga16_get<DT, V>(xv[u][t], i), a * cc);
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
        ga16_store<DT, V, W, NT>(out + p.pair * F, l, F, nT, acc);  // ONE rounding per element
        if (l == 0) *reinterpret_cast<float2*>(stats + 2 * p.pair) = make_float2(m, lsum);
    }
}

// ---- backward, row pass
template <int DT, int V, int W, bool DROP, bool PART>
__global__ __launch_bounds__(kThreads) void gatv2_attention_backward_row_x16_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind, const uint16_t* __restrict__ xl, const uint16_t* __restrict__ xr,
    const float* __restrict__ att, const float* __restrict__ stats, const uint16_t* __restrict__ out, const uint16_t* __restrict__ grad_out,
    float* __restrict__ delta, uint16_t* __restrict__ grad_xl, float* __restrict__ att_part, int M, int H, int F, float slope, int leaky_i,
    EdgeDropout drop) {
    constexpr int G = 64 / W;
    constexpr int NT = 8 / V;
    constexpr int UG = kGa16UnrollRow;
    const bool leaky = leaky_i != 0;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / W;
    const int l = lane % W;
    const int P = M * H;
    const int pair0 = (blockIdx.x * kWaves + wave) * G;
    if (pair0 >= P) return;  // whole wavefront
    Ga16Drop dw = {};
    if constexpr (DROP) dw = {drop.seed[0], drop.seed[1], drop.threshold, drop.scale};
    const Ga16Pair p = ga16_pair(rowptr, pair0, g, P, H);
    const int nT = (F + W * V - 1) / (W * V);
    const int ld = H * F;
    const int off = p.h * F;
    float xs[8], as[8], gs[8], acc_x[8], acc_a[8];
    float dl;
    {
        float os[8];  // the STORED out: what the forward rounded
        ga16_load_wide<DT, V, W, NT>(grad_out + p.pair * F, l, F, nT, gs);
        ga16_load_wide<DT, V, W, NT>(out + p.pair * F, l, F, nT, os);
        dl = ga16_butterfly<W>(ga16_chain_wide<V, NT>(gs, os, nT));
    }
    ga16_load_wide<DT, V, W, NT>(xl + p.pair * F, l, F, nT, xs);
    ga16_load_f32<V, W, NT>(att + off, l, F, nT, as);
    const float2 ml = *reinterpret_cast<const float2*>(stats + 2 * p.pair);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        acc_x[j] = 0.0f;
        acc_a[j] = 0.0f;
    }
    for (int p0 = 0; p0 < p.dmax; p0 += W) {
        const int c = ga16_index(colind, p, p0 + l);
        const int kmax = (p.dmax - p0 < W) ? p.dmax - p0 : W;
        for (int k0 = 0; k0 < kmax; k0 += UG) {
            Ga16Vec<V> xv[UG][NT];
            int ck[UG];
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                ck[u] = __shfl(c, k0 + u, W);
                ga16_load<V, W, NT>(xr + ck[u] * ld + off, l, F, nT, xv[u]);
            }
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                const bool valid = p0 + k0 + u < p.d;
                const float s = ga16_butterfly<W>(ga16_score_chain<DT, V, NT>(as, xs, xv[u], nT, slope, leaky));
                float gp = ga16_butterfly<W>(ga16_chain<DT, V, NT>(gs, xv[u], nT));
                if constexpr (DROP)
                    gp = edge_dropout_apply(gp, edge_dropout_bits(dw.s0, dw.s1, (uint32_t)p.seg, (uint32_t)ck[u], (uint32_t)p.h), dw.threshold,
                                            dw.scale);
                const float a = __expf(s - ml.x) / ml.y;
                const float ds = a * (gp - dl);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
#pragma unroll
                    for (int i = 0; i < V; ++i) {
                        const int j = t * V + i;
                        const float tt = xs[j] + ga16_get<DT, V>(xv[u][t], i);
                        const bool neg = leaky && !(tt >= 0.0f);
                        const float ai = as[j];
                        const float mf = neg ? ai * slope : ai;
                        const float ox = acc_x[j];
                        const float nx = __builtin_fmaf(ds, mf, ox);
                        acc_x[j] = valid ? nx : ox;
                        if constexpr (PART) {
                            const float oa = acc_a[j];
                            const float na = __builtin_fmaf(ds, neg ? slope * tt : tt, oa);
                            acc_a[j] = valid ? na : oa;
                        }
                    }
                }
            }
        }
    }
    if (p.live) {
        ga16_store<DT, V, W, NT>(grad_xl + p.pair * F, l, F, nT, acc_x);  // ONE rounding per element
        if constexpr (PART) ga16_store_f32<V, W, NT>(att_part + p.pair * F, l, F, nT, acc_a);
        if (l == 0) delta[p.pair] = dl;
    }
}

// ---- backward, column pass: segment = column c of the pattern, index = row r
template <int DT, int V, int W, bool DROP>
__global__ __launch_bounds__(kThreads) void gatv2_attention_backward_col_x16_kernel(
    const int32_t* __restrict__ colptr, const int32_t* __restrict__ rowind, const uint16_t* __restrict__ xl, const uint16_t* __restrict__ xr,
    const float* __restrict__ att, const float* __restrict__ stats, const float* __restrict__ delta, const uint16_t* __restrict__ grad_out,
    uint16_t* __restrict__ grad_xr, int K, int H, int F, float slope, int leaky_i, EdgeDropout drop) {
    constexpr int G = 64 / W;
    constexpr int NT = 8 / V;
    constexpr int UG = kGa16UnrollCol;
    const bool leaky = leaky_i != 0;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / W;
    const int l = lane % W;
    const int P = K * H;
    const int pair0 = (blockIdx.x * kWaves + wave) * G;
    if (pair0 >= P) return;  // whole wavefront
    Ga16Drop dw = {};
    if constexpr (DROP) dw = {drop.seed[0], drop.seed[1], drop.threshold, drop.scale};
    const Ga16Pair p = ga16_pair(colptr, pair0, g, P, H);
    const int nT = (F + W * V - 1) / (W * V);
    float xs[8], as[8], acc1[8], acc2[8];
    ga16_load_wide<DT, V, W, NT>(xr + p.pair * F, l, F, nT, xs);
    ga16_load_f32<V, W, NT>(att + p.h * F, l, F, nT, as);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        acc1[j] = 0.0f;
        acc2[j] = 0.0f;
    }
    for (int p0 = 0; p0 < p.dmax; p0 += W) {
        const int r = ga16_index(rowind, p, p0 + l);
        const int kmax = (p.dmax - p0 < W) ? p.dmax - p0 : W;
        for (int k0 = 0; k0 < kmax; k0 += UG) {
            Ga16Vec<V> xv[UG][NT], ov[UG][NT];
            float2 ml[UG];
            float dl[UG];
            int rk[UG];
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                rk[u] = __shfl(r, k0 + u, W);
                const int rp = rk[u] * H + p.h;  // the pair of the entry's row
                ga16_load<V, W, NT>(xl + rp * F, l, F, nT, xv[u]);
                ga16_load<V, W, NT>(grad_out + rp * F, l, F, nT, ov[u]);
                ml[u] = *reinterpret_cast<const float2*>(stats + 2 * rp);
                dl[u] = delta[rp];
            }
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                const bool valid = p0 + k0 + u < p.d;
                const float s = ga16_butterfly<W>(ga16_score_chain<DT, V, NT>(as, xs, xv[u], nT, slope, leaky));
                float gp = ga16_butterfly<W>(ga16_chain<DT, V, NT>(xs, ov[u], nT));
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
                        const float tt = ga16_get<DT, V>(xv[u][t], i) + xs[j];
                        const bool neg = leaky && !(tt >= 0.0f);
                        const float ai = as[j];
                        const float mf = neg ? ai * slope : ai;
                        const float o1 = acc1[j], o2 = acc2[j];
                        const float n1 = __builtin_fmaf(ds, mf, o1);
                        const float n2 = __builtin_fmaf(av, ga16_get<DT, V>(ov[u][t], i), o2);
                        acc1[j] = valid ? n1 : o1;
                        acc2[j] = valid ? n2 : o2;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc1[j] = acc1[j] + acc2[j];  // the ONE add of the two chains; the store rounds it once
    if (p.live) ga16_store<DT, V, W, NT>(grad_xr + p.pair * F, l, F, nT, acc1);
}

// blocks that cover `pairs` (segment, head) pairs with 64 / W lane groups per wavefront
inline int ga16_blocks(int64_t pairs, int W) {
    const int64_t per_block = (int64_t)kWaves * (64 / W);
    return (int)((pairs + per_block - 1) / per_block);
}

// One switch over (V, W, dropout) for the three kernels (GESPMM_GA_SWITCH of gatv2_attention.hip with the type in front): KERNEL is the
// template's name and its arguments after (DT, V, W, DROP) — in parentheses, with a leading comma, or empty — the rest the kernel's
// arguments before `drop`.
#define GESPMM_GA16_UNWRAP(...) __VA_ARGS__
#define GESPMM_GA16_CASE(KERNEL, EXTRA, VV, WW, PAIRS, ...)                                                                               \
    case VV * 100 + WW:                                                                                                                   \
        if (drop)                                                                                                                         \
            hipLaunchKernelGGL((KERNEL<DT, VV, WW, true GESPMM_GA16_UNWRAP EXTRA>), dim3(ga16_blocks(PAIRS, WW)), dim3(kThreads), 0, st,  \
                               __VA_ARGS__, *drop);                                                                                       \
        else                                                                                                                              \
            hipLaunchKernelGGL((KERNEL<DT, VV, WW, false GESPMM_GA16_UNWRAP EXTRA>), dim3(ga16_blocks(PAIRS, WW)), dim3(kThreads), 0, st, \
                               __VA_ARGS__, EdgeDropout{});                                                                               \
        return hipGetLastError();
#define GESPMM_GA16_SWITCH(KERNEL, EXTRA, PAIRS, ...)                   \
    switch (r.V * 100 + r.W) {                                          \
        GESPMM_GA16_CASE(KERNEL, EXTRA, 1, 4, PAIRS, __VA_ARGS__)       \
        GESPMM_GA16_CASE(KERNEL, EXTRA, 1, 8, PAIRS, __VA_ARGS__)       \
        GESPMM_GA16_CASE(KERNEL, EXTRA, 1, 16, PAIRS, __VA_ARGS__)      \
        GESPMM_GA16_CASE(KERNEL, EXTRA, 1, 32, PAIRS, __VA_ARGS__)      \
        GESPMM_GA16_CASE(KERNEL, EXTRA, 1, 64, PAIRS, __VA_ARGS__)      \
        GESPMM_GA16_CASE(KERNEL, EXTRA, 2, 4, PAIRS, __VA_ARGS__)       \
        GESPMM_GA16_CASE(KERNEL, EXTRA, 2, 8, PAIRS, __VA_ARGS__)       \
        GESPMM_GA16_CASE(KERNEL, EXTRA, 2, 16, PAIRS, __VA_ARGS__)      \
        GESPMM_GA16_CASE(KERNEL, EXTRA, 2, 32, PAIRS, __VA_ARGS__)      \
        GESPMM_GA16_CASE(KERNEL, EXTRA, 2, 64, PAIRS, __VA_ARGS__)      \
        GESPMM_GA16_CASE(KERNEL, EXTRA, 4, 4, PAIRS, __VA_ARGS__)       \
        GESPMM_GA16_CASE(KERNEL, EXTRA, 4, 8, PAIRS, __VA_ARGS__)       \
        GESPMM_GA16_CASE(KERNEL, EXTRA, 4, 16, PAIRS, __VA_ARGS__)      \
        GESPMM_GA16_CASE(KERNEL, EXTRA, 4, 32, PAIRS, __VA_ARGS__)      \
        GESPMM_GA16_CASE(KERNEL, EXTRA, 4, 64, PAIRS, __VA_ARGS__)      \
    }                                                                   \
    return hipErrorInvalidValue;

// Sizes the kernels' 32-bit element positions hold, and a launch shape that covers the slice with 8 elements per lane.
bool ga16_launchable(int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, const Gatv2AttentionLaunch& r,
                     const EdgeDropout* drop) {
    if (dtype != kX16F16 && dtype != kX16Bf16) return false;
    if (nnz < 1 || M < 1 || K < 1 || H < 1 || F < 1 || F > kGatv2AttentionMaxF || !r.supported) return false;
    if (nnz > kSddmmMaxNnz || M > kSddmmMaxNnz / H || K > kSddmmMaxNnz / H || M * H > kSddmmMaxNnz / F || K * H > kSddmmMaxNnz / F ||
        M * H > kSddmmMaxNnz / 2)
        return false;
    if ((r.V != 1 && r.V != 2 && r.V != 4) || (F % r.V) != 0 || r.W < 4 || r.W > 64 || (r.W & (r.W - 1)) != 0 || 8 * (int64_t)r.W < F)
        return false;
    return !(drop && !drop->seed);
}

template <int DT>
hipError_t ga16_forward(const int32_t* rowptr, const int32_t* colind, const uint16_t* xl, const uint16_t* xr, const float* att, uint16_t* out,
                        float* stats, int64_t M, int64_t H, int64_t F, float slope, const Gatv2AttentionLaunch& r, const EdgeDropout* drop,
                        hipStream_t st) {
    const int leaky = slope != 1.0f ? 1 : 0;
    GESPMM_GA16_SWITCH(gatv2_attention_x16_kernel, (), M * H, rowptr, colind, xl, xr, att, out, stats, (int)M, (int)H, (int)F, slope, leaky)
}

template <int DT>
hipError_t ga16_row_part(const int32_t* rowptr, const int32_t* colind, const uint16_t* xl, const uint16_t* xr, const float* att,
                         const float* stats, const uint16_t* out, const uint16_t* grad_out, float* delta, uint16_t* grad_xl, float* att_part,
                         int64_t M, int64_t H, int64_t F, float slope, const Gatv2AttentionLaunch& r, const EdgeDropout* drop,
                         hipStream_t st) {
    const int leaky = slope != 1.0f ? 1 : 0;
    GESPMM_GA16_SWITCH(gatv2_attention_backward_row_x16_kernel, (, true), M * H, rowptr, colind, xl, xr, att, stats, out, grad_out, delta,
                       grad_xl, att_part, (int)M, (int)H, (int)F, slope, leaky)
}

template <int DT>
hipError_t ga16_row_plain(const int32_t* rowptr, const int32_t* colind, const uint16_t* xl, const uint16_t* xr, const float* att,
                          const float* stats, const uint16_t* out, const uint16_t* grad_out, float* delta, uint16_t* grad_xl, int64_t M,
                          int64_t H, int64_t F, float slope, const Gatv2AttentionLaunch& r, const EdgeDropout* drop, hipStream_t st) {
    const int leaky = slope != 1.0f ? 1 : 0;
    float* const none = nullptr;
    GESPMM_GA16_SWITCH(gatv2_attention_backward_row_x16_kernel, (, false), M * H, rowptr, colind, xl, xr, att, stats, out, grad_out, delta,
                       grad_xl, none, (int)M, (int)H, (int)F, slope, leaky)
}

template <int DT>
hipError_t ga16_col(const int32_t* colptr, const int32_t* rowind, const uint16_t* xl, const uint16_t* xr, const float* att,
                    const float* stats, const float* delta, const uint16_t* grad_out, uint16_t* grad_xr, int64_t K, int64_t H, int64_t F,
                    float slope, const Gatv2AttentionLaunch& r, const EdgeDropout* drop, hipStream_t st) {
    const int leaky = slope != 1.0f ? 1 : 0;
    GESPMM_GA16_SWITCH(gatv2_attention_backward_col_x16_kernel, (), K * H, colptr, rowind, xl, xr, att, stats, delta, grad_out, grad_xr,
                       (int)K, (int)H, (int)F, slope, leaky)
}

inline const uint16_t* u16(const void* p) { return static_cast<const uint16_t*>(p); }
inline uint16_t* u16(void* p) { return static_cast<uint16_t*>(p); }

}  // namespace

hipError_t launch_gatv2_attention_x16(const int32_t* rowptr, const int32_t* colind, const void* xl, const void* xr, const float* att,
                                      void* out, float* stats, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz,
                                      float slope, const Gatv2AttentionLaunch& r, const EdgeDropout* drop, hipStream_t st) {
    if (!ga16_launchable(dtype, M, K, H, F, nnz, r, drop)) return hipErrorInvalidValue;
    if (dtype == kX16F16) return ga16_forward<kX16F16>(rowptr, colind, u16(xl), u16(xr), att, u16(out), stats, M, H, F, slope, r, drop, st);
    return ga16_forward<kX16Bf16>(rowptr, colind, u16(xl), u16(xr), att, u16(out), stats, M, H, F, slope, r, drop, st);
}

hipError_t launch_gatv2_attention_backward_row_x16(const int32_t* rowptr, const int32_t* colind, const void* xl, const void* xr,
                                                   const float* att, const float* stats, const void* out, const void* grad_out,
                                                   float* delta, void* grad_xl, float* att_part, int dtype, int64_t M, int64_t K,
                                                   int64_t H, int64_t F, int64_t nnz, float slope, const Gatv2AttentionLaunch& r,
                                                   const EdgeDropout* drop, hipStream_t st) {
    if (!ga16_launchable(dtype, M, K, H, F, nnz, r, drop)) return hipErrorInvalidValue;
    if (dtype == kX16F16) {
        if (att_part)
            return ga16_row_part<kX16F16>(rowptr, colind, u16(xl), u16(xr), att, stats, u16(out), u16(grad_out), delta, u16(grad_xl), att_part,
                                          M, H, F, slope, r, drop, st);
        return ga16_row_plain<kX16F16>(rowptr, colind, u16(xl), u16(xr), att, stats, u16(out), u16(grad_out), delta, u16(grad_xl), M, H, F,
                                       slope, r, drop, st);
    }
    if (att_part)
        return ga16_row_part<kX16Bf16>(rowptr, colind, u16(xl), u16(xr), att, stats, u16(out), u16(grad_out), delta, u16(grad_xl), att_part, M,
                                       H, F, slope, r, drop, st);
    return ga16_row_plain<kX16Bf16>(rowptr, colind, u16(xl), u16(xr), att, stats, u16(out), u16(grad_out), delta, u16(grad_xl), M, H, F, slope,
                                    r, drop, st);
}

hipError_t launch_gatv2_attention_backward_col_x16(const int32_t* colptr, const int32_t* rowind, const void* xl, const void* xr,
                                                   const float* att, const float* stats, const float* delta, const void* grad_out,
                                                   void* grad_xr, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz,
                                                   float slope, const Gatv2AttentionLaunch& r, const EdgeDropout* drop, hipStream_t st) {
    if (!ga16_launchable(dtype, M, K, H, F, nnz, r, drop)) return hipErrorInvalidValue;
    if (dtype == kX16F16)
        return ga16_col<kX16F16>(colptr, rowind, u16(xl), u16(xr), att, stats, delta, u16(grad_out), u16(grad_xr), K, H, F, slope, r, drop, st);
    return ga16_col<kX16Bf16>(colptr, rowind, u16(xl), u16(xr), att, stats, delta, u16(grad_out), u16(grad_xr), K, H, F, slope, r, drop, st);
}

}  // namespace gespmm
