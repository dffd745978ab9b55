// edge_softmax.hip — the edge softmax over CSR rows and its backward on fp32 (gfx950), the same two with the additive score of a
// graph attention layer computed in place (el[row] + er[col]: no score array), and the per-segment sum of an edge array. Contract, lane
// geometry and the pinned summation order: edge_softmax.h.
//
// Safety rules this file keeps: every load of rowptr / score / alpha / grad_alpha / colind / order / el / er is clamped to a valid
// position (a lane past its row's end re-reads the row's first entry, a lane group without a pair reads word h of entry 0 and of its
// wavefront's first row) and dropped by a select; loop trip counts and the register / sweep choice are wave-uniform (made so with
// readfirstlane), so no load and no cross-lane move sits under a divergent branch; only stores are predicated. A wavefront past M
// returns whole.

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

template <bool LEAKY>
__device__ __forceinline__ float leaky(float x, float slope) {
    if constexpr (LEAKY) return x >= 0.0f ? x : slope * x;
    return x;
}

// ---- where the value of entry e, head h comes from: a source trait (the operand-trait pattern of sddmm_edge.h) over the three
// pointers (idx, a, b) a launch hands it. row() is what a pair loads once, at(..) the value of one entry; e is a valid entry,
// w = e H + h its word. The pointers travel as __restrict__ parameters of the pair functions, not inside the trait.
//
// kInPlace: the forward reads a[word] in its own loop body, not through at(). Behind a call — a trait's or a lambda's, inlined or
// not — hipcc schedules the sweeps of the forward differently (65 VGPRs for 44, occupancy 7 for 8; measured 1.1-1.6x slower on the
// swept rows of products-sbm); read in place, the code of the array source is the one it was before there were sources.
#define GESPMM_SRC_PTRS const int32_t *__restrict__ idx, const float *__restrict__ a, const float *__restrict__ b
struct EdgeArray {  // a: an [nnz, H] array in edge order — the score, or the x of a segment sum
    static constexpr bool kInPlace = true;
    struct Row {};
    static __device__ __forceinline__ Row row(GESPMM_SRC_PTRS, int, int, int) { return {}; }
    static __device__ __forceinline__ float at(GESPMM_SRC_PTRS, Row, int, int w, int, int) { return a[w]; }
};
struct PermutedEdgeArray {  // the same through a permutation of the entries: a[idx[e], h]
    static constexpr bool kInPlace = false;
    struct Row {};
    static __device__ __forceinline__ Row row(GESPMM_SRC_PTRS, int, int, int) { return {}; }
    static __device__ __forceinline__ float at(GESPMM_SRC_PTRS, Row, int e, int, int h, int H) { return a[idx[e] * H + h]; }
};
// a = el, b = er, idx = colind: el[row, h] + er[colind[e], h], one plain fp32 add — the fl(el + er) the width-2 SDDMM writes. el is
// loaded once per pair, colind and er once per entry and sweep (M H and K H words: 32-bit positions).
struct AddedScore {
    static constexpr bool kInPlace = false;
    struct Row {
        float el;
    };
    static __device__ __forceinline__ Row row(GESPMM_SRC_PTRS, int r, int h, int H) { return {a[r * H + h]}; }
    static __device__ __forceinline__ float at(GESPMM_SRC_PTRS, Row x, int e, int, int h, int H) { return x.el + b[idx[e] * H + h]; }
};

// One (row, head) pair per lane group: the row's d entries start at entry lo, lane l of the W takes entries l + t W. All 64 lanes
// arrive together; d is uniform in the group, d == 0 (then lo == 0) means the group has nothing to do and only keeps the others company.
// row is the pair's row (a valid one for an idle group): what SRC::row reads. A row longer than IT W asks the source again in every sweep.
template <int W, bool LEAKY, class SRC>
__device__ __forceinline__ void softmax_pair(GESPMM_SRC_PTRS, float* __restrict__ out, int row, int lo, int d, int h, int H, int l,
                                             float slope) {
    const int dm = wave_max_degree<W>(d);
    if (dm == 0) return;
    auto word = [&](int p) { return (lo + (p < d ? p : 0)) * H + h; };  // (nnz H <= kSddmmMaxNnz: 32-bit word positions)
    auto entry = [&](int p) { return lo + (p < d ? p : 0); };
    const typename SRC::Row sr = SRC::row(idx, a, b, row, h, H);
    if (dm <= IT * W) {
        float x[IT], t[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            x[it] = -INFINITY;
            if (it * W < dm) {  // wave-uniform
                const int p = l + it * W;
                float v;  // (kInPlace: see EdgeArray)
                if constexpr (SRC::kInPlace) v = a[word(p)];
                else v = SRC::at(idx, a, b, sr, entry(p), word(p), h, H);
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
            float v;  // (kInPlace: see EdgeArray)
            if constexpr (SRC::kInPlace) v = a[word(p)];
            else v = SRC::at(idx, a, b, sr, entry(p), word(p), h, H);
            m = fmaxf(m, p < d ? leaky<LEAKY>(v, slope) : -INFINITY);
        }
        m = group_max<W>(m);
        float s = 0.0f;
#pragma unroll 4
        for (int k = 0; k < nt; ++k) {
            const int p = l + k * W;
            float v;  // (kInPlace: see EdgeArray)
            if constexpr (SRC::kInPlace) v = a[word(p)];
            else v = SRC::at(idx, a, b, sr, entry(p), word(p), h, H);
            s += p < d ? __expf(leaky<LEAKY>(v, slope) - m) : 0.0f;
        }
        s = group_sum<W>(s);
#pragma unroll 4
        for (int k = 0; k < nt; ++k) {
            const int p = l + k * W;
            float v;  // (kInPlace: see EdgeArray)
            if constexpr (SRC::kInPlace) v = a[word(p)];
            else v = SRC::at(idx, a, b, sr, entry(p), word(p), h, H);
            if (p < d) out[word(p)] = __expf(leaky<LEAKY>(v, slope) - m) / s;
        }
    }
}

// The pair's row maximum m and row sum s of exp(x - m), and nothing else: softmax_pair without its third pass, statement for
// statement — both regimes, the same fmaxf chain and butterfly, the same `s += t` chain in which a masked position adds +0 — so
// (m, s) carry the bits softmax_pair divides by. A function of its own, not a helper softmax_pair calls: behind a call hipcc
// schedules the forward's sweeps differently (see kInPlace above). A pair without entries answers (+0, +0).
template <int W, bool LEAKY, class SRC>
__device__ __forceinline__ float2 stats_pair(GESPMM_SRC_PTRS, int row, int lo, int d, int h, int H, int l, float slope) {
    const int dm = wave_max_degree<W>(d);
    if (dm == 0) return make_float2(0.0f, 0.0f);
    auto word = [&](int p) { return (lo + (p < d ? p : 0)) * H + h; };
    auto entry = [&](int p) { return lo + (p < d ? p : 0); };
    const typename SRC::Row sr = SRC::row(idx, a, b, row, h, H);
    float m = -INFINITY, s = 0.0f;
    if (dm <= IT * W) {
        float x[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            x[it] = -INFINITY;
            if (it * W < dm) {  // wave-uniform
                const int p = l + it * W;
                const float v = SRC::at(idx, a, b, sr, entry(p), word(p), h, H);
                x[it] = p < d ? leaky<LEAKY>(v, slope) : -INFINITY;
            }
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) m = fmaxf(m, x[it]);
        m = group_max<W>(m);
#pragma unroll
        for (int it = 0; it < IT; ++it) s += (l + it * W < d) ? __expf(x[it] - m) : 0.0f;
        s = group_sum<W>(s);
    } else {
        const int nt = (dm + W - 1) / W;  // wave-uniform
#pragma unroll 4
        for (int k = 0; k < nt; ++k) {
            const int p = l + k * W;
            const float v = SRC::at(idx, a, b, sr, entry(p), word(p), h, H);
            m = fmaxf(m, p < d ? leaky<LEAKY>(v, slope) : -INFINITY);
        }
        m = group_max<W>(m);
#pragma unroll 4
        for (int k = 0; k < nt; ++k) {
            const int p = l + k * W;
            const float v = SRC::at(idx, a, b, sr, entry(p), word(p), h, H);
            s += p < d ? __expf(leaky<LEAKY>(v, slope) - m) : 0.0f;
        }
        s = group_sum<W>(s);
    }
    return d > 0 ? make_float2(m, s) : make_float2(0.0f, 0.0f);  // (a group without entries beside one with: -inf and 0 are not stored)
}

// ROWSUM: the return value is the sum of the pair's grad values AS STORED, in the pinned order (edge_softmax.h) — plain adds from +0, a
// masked position adds +0, in both regimes; 0 otherwise. The sign of the score comes from SRC (LEAKY only).
template <int W, bool LEAKY, bool ROWSUM, class SRC>
__device__ __forceinline__ float softmax_backward_pair(const float* __restrict__ alpha, const float* __restrict__ galpha, GESPMM_SRC_PTRS,
                                                       float* __restrict__ grad, int row, int lo, int d, int h, int H, int l, float slope) {
    const int dm = wave_max_degree<W>(d);
    if (dm == 0) return 0.0f;
    auto word = [&](int p) { return (lo + (p < d ? p : 0)) * H + h; };
    auto entry = [&](int p) { return lo + (p < d ? p : 0); };
    typename SRC::Row sr{};
    if constexpr (LEAKY) sr = SRC::row(idx, a, b, row, h, H);
    float rs = 0.0f;
    if (dm <= IT * W) {
        float al[IT], g[IT], f[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            al[it] = g[it] = 0.0f;
            f[it] = 1.0f;
            if (it * W < dm) {  // wave-uniform
                const int w = word(l + it * W);
                al[it] = alpha[w];
                g[it] = galpha[w];
                if constexpr (LEAKY) f[it] = SRC::at(idx, a, b, sr, entry(l + it * W), word(l + it * W), h, H) >= 0.0f ? 1.0f : slope;
            }
        }
        float dot = 0.0f;
#pragma unroll
        for (int it = 0; it < IT; ++it) dot = (l + it * W < d) ? fmaf(al[it], g[it], dot) : dot;
        dot = group_sum<W>(dot);
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            float r = al[it] * (g[it] - dot);
            if constexpr (LEAKY) r *= f[it];
            if (l + it * W < d) grad[word(l + it * W)] = r;
            if constexpr (ROWSUM) rs += (l + it * W < d) ? r : 0.0f;
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
            if constexpr (LEAKY) r *= SRC::at(idx, a, b, sr, entry(p), word(p), h, H) >= 0.0f ? 1.0f : slope;
            if (p < d) grad[w] = r;
            if constexpr (ROWSUM) rs += p < d ? r : 0.0f;
        }
    }
    if constexpr (ROWSUM) rs = group_sum<W>(rs);
    return rs;
}

// The sum of the pair's source values in the same pinned order: one loop, the entries asked for once.
template <int W, class SRC>
__device__ __forceinline__ float sum_pair(GESPMM_SRC_PTRS, int row, int lo, int d, int h, int H, int l) {
    const int dm = wave_max_degree<W>(d);
    if (dm == 0) return 0.0f;
    const typename SRC::Row sr = SRC::row(idx, a, b, row, h, H);
    const int nt = (dm + W - 1) / W;  // wave-uniform
    float s = 0.0f;
#pragma unroll 4
    for (int k = 0; k < nt; ++k) {
        const int p = l + k * W;
        const int e = lo + (p < d ? p : 0);
        const float v = SRC::at(idx, a, b, sr, e, e * H + h, h, H);
        s += p < d ? v : 0.0f;
    }
    return group_sum<W>(s);
}

// What a launch does with a pair. row_out ([M, H], every word written: empty rows +0) exists for the last two.
enum Op {
    kForward,      // SRC on (idx, in0, in1) = the score; out = the softmax
    kBackward,     // in0 = alpha, in1 = grad_alpha, SRC on (idx, in2, in3) = the score (LEAKY only, for its sign); out = grad_score
    kBackwardSum,  // ... and row_out = the row sums of grad_score
    kSegmentSum,   // row_out = the row sums of SRC on (idx, in0, in1)
    kStats,        // SRC on (idx, in0, in1) = the score; row_out ([M, H, 2], every word written: empty rows (+0, +0)) = (maximum, sum)
};

template <int W, bool LEAKY, Op OP, class SRC>
__device__ __forceinline__ float pair(const int32_t* __restrict__ idx, const float* __restrict__ in0, const float* __restrict__ in1,
                                      const float* __restrict__ in2, const float* __restrict__ in3, float* __restrict__ out, int row, int lo,
                                      int d, int h, int H, int l, float slope) {
    if constexpr (OP == kForward) {
        softmax_pair<W, LEAKY, SRC>(idx, in0, in1, out, row, lo, d, h, H, l, slope);
        return 0.0f;
    } else if constexpr (OP == kSegmentSum) {
        return sum_pair<W, SRC>(idx, in0, in1, row, lo, d, h, H, l);
    } else {
        return softmax_backward_pair<W, LEAKY, OP == kBackwardSum, SRC>(in0, in1, idx, in2, in3, out, row, lo, d, h, H, l, slope);
    }
}

template <int W, bool LEAKY, Op OP, class SRC>
__global__ __launch_bounds__(kThreads) void edge_softmax_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ idx,
                                                                 const float* __restrict__ in0, const float* __restrict__ in1,
                                                                 const float* __restrict__ in2, const float* __restrict__ in3,
                                                                 float* __restrict__ out, float* __restrict__ row_out, int M, int H, int rpw,
                                                                 int L, float slope) {
    constexpr int G = 64 / W;
    constexpr bool ROWOUT = OP == kBackwardSum || OP == kSegmentSum;
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
        const int ri = (int)(tc / (unsigned)H);  // the pair's row within the wavefront (an idle group: row 0, head 0)
        const int h = (int)(tc - (unsigned)ri * (unsigned)H);
        int lo = __shfl(rp, ri, 64);
        int d = __shfl(rp, ri + 1, 64) - lo;
        const bool mine = act && d <= L;  // (an empty row included: its row_out word is +0)
        if (!act || d <= 0 || d > L) {
            d = 0;
            lo = 0;
        }
        if constexpr (OP == kStats) {  // (its own statement: the other operations' code stays what it was)
            const float2 ms = stats_pair<W, LEAKY, SRC>(idx, in0, in1, r0 + ri, lo, d, h, H, l, slope);
            if (mine && l == 0) reinterpret_cast<float2*>(row_out)[(r0 + ri) * H + h] = ms;  // one 8-byte store (M H <= kSddmmMaxNnz)
        } else {
            const float s = pair<W, LEAKY, OP, SRC>(idx, in0, in1, in2, in3, out, r0 + ri, lo, d, h, H, l, slope);
            if constexpr (ROWOUT)
                if (mine && l == 0) row_out[(r0 + ri) * H + h] = s;  // (M H <= kSddmmMaxNnz)
        }
    }
    // ---- hub rows: a whole wavefront per pair (wave-uniform branch: rp lives in lanes, the row index is a loop counter)
    if (hubs) {
        for (int i = 0; i < nr; ++i) {
            const int lo = __builtin_amdgcn_readlane(rp, i);
            const int d = __builtin_amdgcn_readlane(rp, i + 1) - lo;
            if (d > L)
                for (int h = 0; h < H; ++h) {
                    if constexpr (OP == kStats) {
                        const float2 ms = stats_pair<64, LEAKY, SRC>(idx, in0, in1, r0 + i, lo, d, h, H, lane, slope);
                        if (lane == 0) reinterpret_cast<float2*>(row_out)[(r0 + i) * H + h] = ms;
                    } else {
                        const float s = pair<64, LEAKY, OP, SRC>(idx, in0, in1, in2, in3, out, r0 + i, lo, d, h, H, lane, slope);
                        if constexpr (ROWOUT)
                            if (lane == 0) row_out[(r0 + i) * H + h] = s;
                    }
                }
        }
    }
}

template <bool LEAKY, Op OP, class SRC>
hipError_t launch_w(const int32_t* rowptr, const int32_t* idx, const float* in0, const float* in1, const float* in2, const float* in3,
                    float* out, float* row_out, int M, int H, float slope, const EdgeSoftmaxLaunch& r, hipStream_t st) {
    const int nblk = (int)(((int64_t)M + kWaves * r.rpw - 1) / (kWaves * r.rpw));
#define GESPMM_ES(WW)                                                                                                                 \
    case WW:                                                                                                                           \
        hipLaunchKernelGGL((edge_softmax_kernel<WW, LEAKY, OP, SRC>), dim3(nblk), dim3(kThreads), 0, st, rowptr, idx, in0, in1, in2,   \
                           in3, out, row_out, M, H, r.rpw, r.L, slope);                                                                \
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

// rows x H words of a dense [rows, H] operand or result within 32-bit word positions
bool dense_words_fit(int64_t rows, int64_t H) { return H >= 1 && rows <= kSddmmMaxNnz / H; }

}  // namespace

hipError_t launch_edge_softmax(const int32_t* rowptr, const float* score, float* out, int64_t M, int64_t H, int64_t nnz, float slope,
                               const EdgeSoftmaxLaunch& r, hipStream_t st) {
    if (nnz == 0 || M == 0) return hipSuccess;
    if (!launchable(M, H, nnz, r)) return hipErrorInvalidValue;
    const float* no = nullptr;
    if (slope != 1.0f) return launch_w<true, kForward, EdgeArray>(rowptr, nullptr, score, no, no, no, out, nullptr, (int)M, (int)H, slope, r, st);
    return launch_w<false, kForward, EdgeArray>(rowptr, nullptr, score, no, no, no, out, nullptr, (int)M, (int)H, slope, r, st);
}

hipError_t launch_edge_softmax_backward(const int32_t* rowptr, const float* alpha, const float* grad_alpha, const float* score,
                                        float* grad_score, int64_t M, int64_t H, int64_t nnz, float slope, const EdgeSoftmaxLaunch& r,
                                        hipStream_t st) {
    if (nnz == 0 || M == 0) return hipSuccess;
    if (!launchable(M, H, nnz, r)) return hipErrorInvalidValue;
    const float* no = nullptr;
    if (slope != 1.0f)
        return launch_w<true, kBackward, EdgeArray>(rowptr, nullptr, alpha, grad_alpha, score, no, grad_score, nullptr, (int)M, (int)H, slope,
                                                    r, st);
    return launch_w<false, kBackward, EdgeArray>(rowptr, nullptr, alpha, grad_alpha, no, no, grad_score, nullptr, (int)M, (int)H, slope, r, st);
}

hipError_t launch_gat_softmax(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, float* out, int64_t M,
                              int64_t K, int64_t H, int64_t nnz, float slope, const EdgeSoftmaxLaunch& r, hipStream_t st) {
    if (nnz == 0 || M == 0) return hipSuccess;
    if (!launchable(M, H, nnz, r) || !dense_words_fit(M, H) || K < 1 || !dense_words_fit(K, H)) return hipErrorInvalidValue;
    const float* no = nullptr;
    if (slope != 1.0f) return launch_w<true, kForward, AddedScore>(rowptr, colind, el, er, no, no, out, nullptr, (int)M, (int)H, slope, r, st);
    return launch_w<false, kForward, AddedScore>(rowptr, colind, el, er, no, no, out, nullptr, (int)M, (int)H, slope, r, st);
}

hipError_t launch_gat_softmax_stats(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, float* stats, int64_t M,
                                    int64_t K, int64_t H, int64_t nnz, float slope, const EdgeSoftmaxLaunch& r, hipStream_t st) {
    if (M == 0) return hipSuccess;
    if (H < 1 || !dense_words_fit(M, H)) return hipErrorInvalidValue;
    if (nnz == 0) return hipMemsetAsync(stats, 0, (size_t)M * (size_t)H * 2 * sizeof(float), st);
    if (!launchable(M, H, nnz, r) || K < 1 || !dense_words_fit(K, H)) return hipErrorInvalidValue;
    const float* no = nullptr;
    if (slope != 1.0f) return launch_w<true, kStats, AddedScore>(rowptr, colind, el, er, no, no, nullptr, stats, (int)M, (int)H, slope, r, st);
    return launch_w<false, kStats, AddedScore>(rowptr, colind, el, er, no, no, nullptr, stats, (int)M, (int)H, slope, r, st);
}

hipError_t launch_gat_softmax_backward(const int32_t* rowptr, const int32_t* colind, const float* alpha, const float* grad_alpha,
                                       const float* el, const float* er, float* grad_score, float* grad_el, int64_t M, int64_t K, int64_t H,
                                       int64_t nnz, float slope, const EdgeSoftmaxLaunch& r, hipStream_t st) {
    if (M == 0) return hipSuccess;
    if (H < 1 || !dense_words_fit(M, H)) return hipErrorInvalidValue;
    if (nnz == 0) return hipMemsetAsync(grad_el, 0, (size_t)M * (size_t)H * sizeof(float), st);
    if (!launchable(M, H, nnz, r)) return hipErrorInvalidValue;
    if (slope != 1.0f) {
        if (K < 1 || !dense_words_fit(K, H)) return hipErrorInvalidValue;
        return launch_w<true, kBackwardSum, AddedScore>(rowptr, colind, alpha, grad_alpha, el, er, grad_score, grad_el, (int)M, (int)H,
                                                        slope, r, st);
    }
    return launch_w<false, kBackwardSum, EdgeArray>(rowptr, nullptr, alpha, grad_alpha, nullptr, nullptr, grad_score, grad_el, (int)M, (int)H,
                                                    slope, r, st);
}

hipError_t launch_edge_segment_sum(const int32_t* ptr, const int32_t* order, const float* x, float* out, int64_t S, int64_t H, int64_t nnz,
                                   const EdgeSoftmaxLaunch& r, hipStream_t st) {
    if (S == 0) return hipSuccess;
    if (H < 1 || !dense_words_fit(S, H)) return hipErrorInvalidValue;
    if (nnz == 0) return hipMemsetAsync(out, 0, (size_t)S * (size_t)H * sizeof(float), st);
    if (!launchable(S, H, nnz, r)) return hipErrorInvalidValue;
    const float* no = nullptr;
    if (order) return launch_w<false, kSegmentSum, PermutedEdgeArray>(ptr, order, x, no, no, no, nullptr, out, (int)S, (int)H, 1.0f, r, st);
    return launch_w<false, kSegmentSum, EdgeArray>(ptr, nullptr, x, no, no, no, nullptr, out, (int)S, (int)H, 1.0f, r, st);
}

}  // namespace gespmm
