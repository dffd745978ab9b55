// gat_backward.hip — grad_el and grad_er of a graph attention layer without an edge-sized array (gat_backward.h: contract, lane
// geometry, pinned orders). ONE kernel template for both passes: TRANSPOSED = false walks the rows (writes delta and grad_el),
// TRANSPOSED = true the columns (reads delta, writes grad_er). A translation unit of its own: edge_softmax_kernel and
// gat_aggregate_kernel stay exactly what they are; the lane geometry and the chains are restated here, statement for statement
// (group_sum and wave_max_degree are edge_softmax.h's).
//
// Safety rules (those of edge_softmax.hip): every load of ptr / ind / el / er / stats / delta / grad_out / feat is of a valid word —
// a lane past its segment's end re-reads the segment's first entry, a lane group without a pair reads entry 0 and its wavefront's
// first segment — and what it yields is dropped by a select; loop trip counts and the register / sweep choice are wave-uniform (made
// so with readfirstlane), so no load and no cross-lane move sits under a divergent branch; only stores are predicated. A wavefront
// past S returns whole.
//
// The fixed operand of a pair (grad_out[r, h, :] in the row pass, feat[c, h, :] in the column pass) is read through broadcast loads:
// the W lanes of a group ask for the same 16 bytes, which one L1 line serves. F is a run-time value, so registers would need a
// kernel per F; LDS would need rpw H F words per wavefront (16 KiB at H F = 64 x 64 pairs: 64 KiB per workgroup, two workgroups per
// CU) for an operand the L1 already holds.

#include "gat_backward.h"

#include <math.h>

#include "edge_dropout.h"
#include "edge_softmax.h"
#include "gat_aggregate.h"
#include "spmm_kernels.h"

namespace gespmm {
namespace {

constexpr int IT = kEdgeSoftmaxIT;  // entries a lane keeps in registers

template <int V>
__device__ __forceinline__ void load_words(float (&v)[V], const float* __restrict__ p) {
    if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
        v[0] = p[0];
    }
}

// DROP (gespmm_gat_backward_{el,er}_dropout_f32; edge_dropout.h): the dot becomes g'_p = dropout(g_p) directly after its chain — one
// rounding fl(g s), or +0 by a select — and every statement after it is unchanged (w_p stays the undropped weight). The entry's (row,
// column) is (segment, index) in the row pass and (index, segment) in the column pass: the same pair, hence the same decision. The
// seed's two words are loaded once per wavefront, uniformly; everything of it sits behind `if constexpr`.
struct DropWords {
    uint32_t s0, s1, threshold;
    float scale;
};

// The operands of a launch. fixed / gathered: [S, H, F] of the segments' side and [*, H, F] of the side ind points into — grad_out and
// feat in the row pass, feat and grad_out in the column pass. delta: read in the column pass only.
#define GESPMM_GB_PTRS                                                                                                                \
    const int32_t *__restrict__ ind, const float *__restrict__ el, const float *__restrict__ er, const float2 *__restrict__ stats,    \
        const float *__restrict__ delta, const float *__restrict__ fixed, const float *__restrict__ gathered
#define GESPMM_GB_ARGS ind, el, er, stats, delta, fixed, gathered

// One (segment, head) pair per lane group -> (delta, sum of gs): the segment's d entries start at entry lo, lane l of the W takes
// entries l + t W. All 64 lanes arrive together; d is uniform in the group, d == 0 (then lo == 0) means the group has nothing to do and
// only keeps the others company. seg is a valid segment for an idle group too. V: words per load of the F-wide rows.
template <int W, bool LEAKY, bool TRANSPOSED, int V, bool DROP>
__device__ __forceinline__ float2 backward_pair(GESPMM_GB_PTRS, int seg, int lo, int d, int h, int H, int F, int l, float slope,
                                                const DropWords& dw) {
    const int dm = wave_max_degree<W>(d);
    if (dm == 0) return make_float2(0.0f, 0.0f);
    const int sw = seg * H + h;  // the pair's word (M H, K H, M H F and K H F <= kSddmmMaxNnz: 32-bit word positions)
    const float* __restrict__ fx = fixed + sw * F;
    float el_s = 0.0f, er_s = 0.0f;
    float2 ms_s = make_float2(0.0f, 1.0f);
    if constexpr (TRANSPOSED) {
        er_s = er[sw];
    } else {
        el_s = el[sw];
        ms_s = stats[sw];  // one 8-byte load
    }
    float w[IT], g[IT], f[IT], dl[IT];
    // Entries l + (k0 + it) W, it < IT: the weight, the dot (one fmaf chain per entry over ascending f, from +0), the leaky ReLU's
    // factor and, in the column pass, the delta of the entry's row. An `it` past the longest segment of the wavefront loads nothing.
    auto batch = [&](int k0) {
        int off[IT];
        uint32_t mb[IT];  // (DROP only) the mask's bits of the entry
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            w[it] = g[it] = dl[it] = 0.0f;
            f[it] = 1.0f;
            off[it] = 0;
            mb[it] = 0;
            if ((k0 + it) * W < dm) {  // wave-uniform
                const int p = l + (k0 + it) * W;
                const int j = ind[lo + (p < d ? p : 0)];
                const int nw = j * H + h;
                if constexpr (DROP)
                    mb[it] = edge_dropout_bits(dw.s0, dw.s1, (uint32_t)(TRANSPOSED ? j : seg), (uint32_t)(TRANSPOSED ? seg : j), (uint32_t)h);
                off[it] = nw * F;
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
            }
        }
#pragma unroll 2
        for (int c = 0; c < F; c += V) {  // (F % V == 0)
            float a[V];
            load_words<V>(a, fx + c);
#pragma unroll
            for (int it = 0; it < IT; ++it)
                if ((k0 + it) * W < dm) {  // wave-uniform
                    float b[V];
                    load_words<V>(b, gathered + off[it] + c);
#pragma unroll
                    for (int i = 0; i < V; ++i) g[it] = fmaf(a[i], b[i], g[it]);
                }
        }
        if constexpr (DROP) {
#pragma unroll
            for (int it = 0; it < IT; ++it) g[it] = edge_dropout_apply(g[it], mb[it], dw.threshold, dw.scale);
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
        dot = group_sum<W>(dot);
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
        dot = group_sum<W>(dot);
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
    rs = group_sum<W>(rs);
    return make_float2(dot, rs);
}

template <int W, bool LEAKY, bool TRANSPOSED, bool DROP>
__device__ __forceinline__ float2 pair(GESPMM_GB_PTRS, int seg, int lo, int d, int h, int H, int F, int l, float slope, bool vec4,
                                       const DropWords& dw) {
    if (vec4) return backward_pair<W, LEAKY, TRANSPOSED, 4, DROP>(GESPMM_GB_ARGS, seg, lo, d, h, H, F, l, slope, dw);  // wave-uniform
    return backward_pair<W, LEAKY, TRANSPOSED, 1, DROP>(GESPMM_GB_ARGS, seg, lo, d, h, H, F, l, slope, dw);
}

// out_delta: [S, H] in the row pass (null in the column pass); out_grad: grad_el [M, H] or grad_er [K, H]. Every word written.
template <int W, bool LEAKY, bool TRANSPOSED, bool DROP>
__device__ __forceinline__ void gat_backward_body(const int32_t* __restrict__ ptr, GESPMM_GB_PTRS, float* __restrict__ out_delta,
                                                  float* __restrict__ out_grad, int S, int H, int F, int rpw, int L, float slope, int vec,
                                                  const EdgeDropout& drop) {
    constexpr int G = 64 / W;
    DropWords dw = {0u, 0u, 0u, 1.0f};
    if constexpr (DROP) dw = {drop.seed[0], drop.seed[1], drop.threshold, drop.scale};  // wave-uniform loads
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / W;
    const int l = lane % W;
    const bool vec4 = vec == 4;                         // kernel argument: wave-uniform
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
        const float2 r = pair<W, LEAKY, TRANSPOSED, DROP>(GESPMM_GB_ARGS, s0 + si, lo, d, h, H, F, l, slope, vec4, dw);
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
                    const float2 r = pair<64, LEAKY, TRANSPOSED, DROP>(GESPMM_GB_ARGS, s0 + i, lo, d, h, H, F, lane, slope, vec4, dw);
                    if (lane == 0) {
                        if constexpr (!TRANSPOSED) out_delta[(s0 + i) * H + h] = r.x;
                        out_grad[(s0 + i) * H + h] = r.y;
                    }
                }
        }
    }
}

template <int W, bool LEAKY, bool TRANSPOSED>
__global__ __launch_bounds__(kThreads) void gat_backward_kernel(const int32_t* __restrict__ ptr, GESPMM_GB_PTRS, float* __restrict__ out_delta,
                                                                 float* __restrict__ out_grad, int S, int H, int F, int rpw, int L,
                                                                 float slope, int vec) {
    gat_backward_body<W, LEAKY, TRANSPOSED, false>(ptr, GESPMM_GB_ARGS, out_delta, out_grad, S, H, F, rpw, L, slope, vec, EdgeDropout{});
}

template <int W, bool LEAKY, bool TRANSPOSED>
__global__ __launch_bounds__(kThreads) void gat_backward_dropout_kernel(const int32_t* __restrict__ ptr, GESPMM_GB_PTRS,
                                                                         float* __restrict__ out_delta, float* __restrict__ out_grad, int S,
                                                                         int H, int F, int rpw, int L, float slope, int vec, EdgeDropout drop) {
    gat_backward_body<W, LEAKY, TRANSPOSED, true>(ptr, GESPMM_GB_ARGS, out_delta, out_grad, S, H, F, rpw, L, slope, vec, drop);
}

template <bool LEAKY, bool TRANSPOSED>
hipError_t launch_w(const int32_t* ptr, const int32_t* ind, const float* el, const float* er, const float* stats, const float* delta,
                    const float* fixed, const float* gathered, float* out_delta, float* out_grad, int S, int H, int F, float slope,
                    const EdgeSoftmaxLaunch& r, const EdgeDropout* drop, hipStream_t st) {
    const int nblk = (int)(((int64_t)S + kWaves * r.rpw - 1) / (kWaves * r.rpw));
    const bool aligned = (reinterpret_cast<uintptr_t>(fixed) | reinterpret_cast<uintptr_t>(gathered)) % 16 == 0;
    const int vec = (F % 4 == 0 && aligned) ? 4 : 1;
#define GESPMM_GB(WW)                                                                                                                   \
    case WW:                                                                                                                            \
        if (drop) {                                                                                                                     \
            hipLaunchKernelGGL((gat_backward_dropout_kernel<WW, LEAKY, TRANSPOSED>), dim3(nblk), dim3(kThreads), 0, st, ptr, ind, el, er, \
                               reinterpret_cast<const float2*>(stats), delta, fixed, gathered, out_delta, out_grad, S, H, F, r.rpw,    \
                               r.L, slope, vec, *drop);                                                                                 \
            return hipGetLastError();                                                                                                   \
        }                                                                                                                               \
        hipLaunchKernelGGL((gat_backward_kernel<WW, LEAKY, TRANSPOSED>), dim3(nblk), dim3(kThreads), 0, st, ptr, ind, el, er,           \
                           reinterpret_cast<const float2*>(stats), delta, fixed, gathered, out_delta, out_grad, S, H, F, r.rpw, r.L,   \
                           slope, vec);                                                                                                 \
        return hipGetLastError();
    switch (r.W) {
        GESPMM_GB(4)
        GESPMM_GB(8)
        GESPMM_GB(16)
    }
#undef GESPMM_GB
    return hipErrorInvalidValue;
}

// rows x H (x F) words of a dense operand or result within 32-bit word positions
bool dense_words_fit(int64_t rows, int64_t H, int64_t F) { return H >= 1 && F >= 1 && rows <= kSddmmMaxNnz / H / F; }

bool launchable(int64_t S, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, const EdgeSoftmaxLaunch& r) {
    return S >= 1 && S <= kEdgeSoftmaxMaxRows && M >= 1 && K >= 1 && H >= 1 && nnz >= 1 && nnz <= kSddmmMaxNnz / H &&
           dense_words_fit(M, H, F) && dense_words_fit(K, H, F) && r.rpw >= 1 && r.rpw <= 63 &&
           (int64_t)r.rpw * H <= (H > 64 ? H : 64) && r.L >= 1;
}

}  // namespace

hipError_t launch_gat_backward_el(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, const float* stats,
                                  const float* grad_out, const float* feat, float* delta, float* grad_el, int64_t M, int64_t K, int64_t H,
                                  int64_t F, int64_t nnz, float slope, const EdgeSoftmaxLaunch& r, const EdgeDropout* drop, hipStream_t st) {
    if (M == 0) return hipSuccess;
    if (!dense_words_fit(M, H, 1)) return hipErrorInvalidValue;
    if (nnz == 0) {
        const hipError_t rc = hipMemsetAsync(delta, 0, (size_t)M * (size_t)H * sizeof(float), st);
        return rc != hipSuccess ? rc : hipMemsetAsync(grad_el, 0, (size_t)M * (size_t)H * sizeof(float), st);
    }
    if (!launchable(M, M, K, H, F, nnz, r) || (drop && !drop->seed)) return hipErrorInvalidValue;
    if (slope != 1.0f)
        return launch_w<true, false>(rowptr, colind, el, er, stats, nullptr, grad_out, feat, delta, grad_el, (int)M, (int)H, (int)F, slope, r, drop, st);
    return launch_w<false, false>(rowptr, colind, el, er, stats, nullptr, grad_out, feat, delta, grad_el, (int)M, (int)H, (int)F, slope, r, drop, st);
}

hipError_t launch_gat_backward_er(const int32_t* colptr, const int32_t* rowind, const float* el, const float* er, const float* stats,
                                  const float* delta, const float* grad_out, const float* feat, float* grad_er, int64_t M, int64_t K,
                                  int64_t H, int64_t F, int64_t nnz, float slope, const EdgeSoftmaxLaunch& r, const EdgeDropout* drop,
                                  hipStream_t st) {
    if (K == 0) return hipSuccess;
    if (!dense_words_fit(K, H, 1)) return hipErrorInvalidValue;
    if (nnz == 0) return hipMemsetAsync(grad_er, 0, (size_t)K * (size_t)H * sizeof(float), st);
    if (!launchable(K, M, K, H, F, nnz, r) || (drop && !drop->seed)) return hipErrorInvalidValue;
    if (slope != 1.0f)
        return launch_w<true, true>(colptr, rowind, el, er, stats, delta, feat, grad_out, nullptr, grad_er, (int)K, (int)H, (int)F, slope, r, drop, st);
    return launch_w<false, true>(colptr, rowind, el, er, stats, delta, feat, grad_out, nullptr, grad_er, (int)K, (int)H, (int)F, slope, r, drop, st);
}

}  // namespace gespmm
