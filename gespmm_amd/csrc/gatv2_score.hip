// gatv2_score.hip — the GATv2 edge score and its gradients on fp32 operands (gfx950). Contract, pinned orders and safety rules:
// gatv2_score.h.
//
//     score[p H + h] = sum_f att[h, f] * leaky(xl[row(p), h, f] + xr[col(p), h, f])        (CSR entry order, head-minor)

#include "gatv2_score.h"

#include "spmm_kernels.h"

namespace gespmm {

namespace {

template <int V> struct Gv2Vec;
template <> struct Gv2Vec<1> { using type = float; };
template <> struct Gv2Vec<2> { using type = float __attribute__((ext_vector_type(2))); };
template <> struct Gv2Vec<4> { using type = float __attribute__((ext_vector_type(4))); };

template <int V> __device__ __forceinline__ float gv2_get(const typename Gv2Vec<V>::type& x, int i) {
    if constexpr (V == 1) return x;
    else return x[i];
}
template <int V> __device__ __forceinline__ void gv2_set(typename Gv2Vec<V>::type& x, int i, float v) {
    if constexpr (V == 1) x = v;
    else x[i] = v;
}

// leaky(t) = t >= 0 ? t : slope * t. `leaky` is false for slope == 1: no multiply.
__device__ __forceinline__ float gv2_leaky(float t, float slope, bool leaky) { return (leaky && !(t >= 0.0f)) ? slope * t : t; }

// Row that owns CSR position e: largest r with rowptr[r] <= e (empty rows skipped).
__device__ __forceinline__ int gv2_row_of_entry(const int32_t* __restrict__ rowptr, int M, int e) {
    int lo = 0, hi = M;  // invariant: rowptr[lo] <= e < rowptr[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rowptr[mid] <= e) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The same for a wavefront-uniform e, all 64 lanes probing at once: every round cuts [lo, hi) into 64 pieces.
__device__ __forceinline__ int gv2_row_of_entry_wave(const int32_t* __restrict__ rowptr, int M, int e, int lane) {
    int lo = 0, hi = M;  // invariant: rowptr[lo] <= e < rowptr[hi]
    while (hi - lo > 1) {
        const int step = (hi - lo + 63) >> 6;
        const int idx = lo + (lane + 1) * step;
        const bool le = idx < hi && rowptr[idx] <= e;  // monotone in the lane: a prefix of the lanes says yes
        const int cnt = __popcll(__ballot(le));
        lo += cnt * step;
        hi = (lo + step < hi) ? lo + step : hi;
    }
    return lo;
}

// ---- forward: the geometry of sddmm_heads_kernel (CSR form) with att's head slice as a third operand.
template <int V, int W>
__global__ __launch_bounds__(kThreads) void gatv2_score_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                                const float* __restrict__ xl, const float* __restrict__ xr,
                                                                const float* __restrict__ att, float* __restrict__ score, int M, int nnz,
                                                                int H, int F, int epw, uint32_t magic, float slope, int leaky_i) {
    constexpr int G = 64 / W;
    constexpr int EPW = 256;  // most entries a wavefront owns (epw <= EPW): one row search per epw entries, their ids in LDS
    constexpr int UE = 4;     // pairs per lane group per step
    using T = typename Gv2Vec<V>::type;
    const bool leaky = leaky_i != 0;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / W;
    const int l = lane % W;

    // ---- the wavefront's entries [e_lo, e_hi), its pairs [e_lo H, e_hi H): ONE wavefront-wide search for the row of the first entry, the
    // epw + 2 row pointers from there in LDS, every lane resolves one entry (the whole-array search when more than epw empty rows fall
    // into the window). The ids are then read H times.
    __shared__ int s_rp[kWaves][EPW + 2];
    __shared__ int s_row[kWaves][EPW];
    __shared__ int s_col[kWaves][EPW];
    const int e_lo = (blockIdx.x * kWaves + wave) * epw;
    if (e_lo >= nnz) return;  // whole wavefront
    const int e_hi = (e_lo + epw < nnz) ? e_lo + epw : nnz;
    const int r0 = gv2_row_of_entry_wave(rowptr, M, e_lo, lane);
    for (int i = lane; i < epw + 2; i += 64) s_rp[wave][i] = (r0 + i <= M) ? rowptr[r0 + i] : 0x7fffffff;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int e = e_lo + lane; e < e_hi; e += 64) {
        int lo = 0;
        if (s_rp[wave][1] <= e) {
            // largest i in [0, epw + 1] with s_rp[i] <= e   (s_rp[0] = rowptr[r0] <= e_lo <= e)
            int hi = epw + 1;
            if (s_rp[wave][hi] <= e) {  // more than epw empty rows in the window: search the whole array
                lo = gv2_row_of_entry(rowptr, M, e) - r0;
                hi = lo + 1;
            }
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_rp[wave][mid] <= e) lo = mid;
                else hi = mid;
            }
        }
        s_row[wave][e - e_lo] = r0 + lo;
        s_col[wave][e - e_lo] = colind[e];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    const int q_lo = e_lo * H, q_hi = e_hi * H;  // (nnz H <= kSddmmMaxNnz: 32-bit pair arithmetic)
    const int ld = H * F;                        // floats between two rows of xl / xr (M H F, K H F <= kSddmmMaxNnz: 32-bit word positions)
    const int nT = (F + W * V - 1) / (W * V);    // vectors per lane and slice: wave-uniform
    for (int rb = 0; rb < q_hi - q_lo; rb += G * UE) {
        const int qbase = q_lo + rb + g * UE;
        // Pair q -> its three head slices. A pair past the wavefront's end takes the last valid pair (re-read, dropped at the store). The
        // entry is t / H on the wavefront-relative pair t < epw H: a host-made multiply-shift where that is exact, else the division.
        int o1[UE], o2[UE], o3[UE];
        float part[UE];
#pragma unroll
        for (int u = 0; u < UE; ++u) {
            const int q = qbase + u;
            const unsigned t = (unsigned)((q < q_hi ? q : q_hi - 1) - q_lo);
            const unsigned er = magic ? __umulhi(t, magic) : t / (unsigned)H;
            const unsigned h = t - er * (unsigned)H;
            o3[u] = (int)h * F;
            o1[u] = s_row[wave][er] * ld + o3[u];
            o2[u] = s_col[wave][er] * ld + o3[u];
            part[u] = 0.0f;
        }
        for (int t = 0; t < nT; ++t) {
            const int j = l * V + t * W * V;
            const bool in = j < F;  // (V divides F: a vector is inside the slice or past it, whole)
            const int jj = in ? j : 0;
            T x[UE], y[UE], a[UE];  // all 3 * UE vectors of the group's UE pairs are requested before any is used
#pragma unroll
            for (int u = 0; u < UE; ++u) {
                x[u] = *reinterpret_cast<const T*>(xl + o1[u] + jj);
                y[u] = *reinterpret_cast<const T*>(xr + o2[u] + jj);
                a[u] = *reinterpret_cast<const T*>(att + o3[u] + jj);
            }
#pragma unroll
            for (int u = 0; u < UE; ++u) {
#pragma unroll
                for (int i = 0; i < V; ++i) {  // a lane past the slice contributes fmaf(0, 0, 0)
                    const float xi = in ? gv2_get<V>(x[u], i) : 0.0f;
                    const float yi = in ? gv2_get<V>(y[u], i) : 0.0f;
                    const float ai = in ? gv2_get<V>(a[u], i) : 0.0f;
                    part[u] = __builtin_fmaf(ai, gv2_leaky(xi + yi, slope, leaky), part[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < UE; ++u) {
#pragma unroll
            for (int m = W >> 1; m > 0; m >>= 1) part[u] += __shfl_xor(part[u], m, 64);
            if (l == 0 && qbase + u < q_hi) score[qbase + u] = part[u];
        }
    }
}

// ---- backward: a group of W lanes walks one segment at width N = H F; one fmaf chain per output word, in segment order.
template <int V, int W, bool PART>
__global__ __launch_bounds__(kThreads) void gatv2_score_backward_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ ind,
                                                                         const int32_t* __restrict__ order,
                                                                         const float* __restrict__ grad_score,
                                                                         const float* __restrict__ x_seg, const float* __restrict__ x_ind,
                                                                         const float* __restrict__ att, float* __restrict__ grad_x,
                                                                         float* __restrict__ att_part, int S, int H, int F, float slope,
                                                                         int leaky_i) {
    constexpr int G = 64 / W;
    constexpr int UG = 4;  // gathers of x_ind rows in flight per lane (W is a multiple of 4)
    using T = typename Gv2Vec<V>::type;
    const bool leaky = leaky_i != 0;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / W;
    const int l = lane % W;
    const int s0 = (blockIdx.x * kWaves + wave) * G;
    if (s0 >= S) return;  // whole wavefront
    const int s = s0 + g;
    const bool live = s < S;  // an idle group walks segment S - 1 as an empty one and stores nothing
    const int sc = live ? s : S - 1;
    const int lo = ptr[sc];
    const int d = live ? ptr[sc + 1] - lo : 0;
    int dmax = d;  // the longest segment among the wavefront's groups: trip counts are wave-uniform
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const int o = __shfl_xor(dmax, m, 64);
        dmax = o > dmax ? o : dmax;
    }
    dmax = __builtin_amdgcn_readfirstlane(dmax);
    const int N = H * F;  // (S H F, T H F <= kSddmmMaxNnz: 32-bit word positions)
    for (int n0 = 0; n0 < N; n0 += W * V) {
        const int n = n0 + l * V;
        const bool okn = n < N;  // (V divides F, hence N: a lane's vector is inside the row or past it, whole, and inside ONE head)
        const int nn = okn ? n : 0;
        const int h = nn / F;
        const T xs = *reinterpret_cast<const T*>(x_seg + sc * N + nn);
        const T a = *reinterpret_cast<const T*>(att + nn);
        T as = a;  // fl(att * slope): the factor of an entry on the negative side
        if (leaky) {
#pragma unroll
            for (int i = 0; i < V; ++i) gv2_set<V>(as, i, gv2_get<V>(a, i) * slope);
        }
        T acc_x = T{}, acc_a = T{};
        for (int p0 = 0; p0 < dmax; p0 += W) {
            // W entries per group, coalesced, then broadcast. A lane past its segment re-reads the segment's first entry (entry 0 where
            // the segment is empty: nnz >= 1); what it gathers is dropped by the select below.
            const int pe = p0 + l;
            const int e = pe < d ? lo + pe : (d > 0 ? lo : 0);
            const int c = ind[e];
            const int q = order ? order[e] : e;
            const int kmax = (dmax - p0 < W) ? dmax - p0 : W;
            for (int k0 = 0; k0 < kmax; k0 += UG) {
                T xv[UG];
                float gv[UG];
#pragma unroll
                for (int u = 0; u < UG; ++u) {
                    const int ck = __shfl(c, k0 + u, W);
                    const int qk = __shfl(q, k0 + u, W);
                    xv[u] = *reinterpret_cast<const T*>(x_ind + ck * N + nn);
                    gv[u] = grad_score[qk * H + h];
                }
#pragma unroll
                for (int u = 0; u < UG; ++u) {
                    const bool valid = p0 + k0 + u < d;
#pragma unroll
                    for (int i = 0; i < V; ++i) {
                        const float t = gv2_get<V>(xs, i) + gv2_get<V>(xv[u], i);
                        const bool neg = leaky && !(t >= 0.0f);
                        const float m = neg ? gv2_get<V>(as, i) : gv2_get<V>(a, i);
                        const float ax = __builtin_fmaf(gv[u], m, gv2_get<V>(acc_x, i));
                        gv2_set<V>(acc_x, i, valid ? ax : gv2_get<V>(acc_x, i));
                        if constexpr (PART) {
                            const float aa = __builtin_fmaf(gv[u], neg ? slope * t : t, gv2_get<V>(acc_a, i));
                            gv2_set<V>(acc_a, i, valid ? aa : gv2_get<V>(acc_a, i));
                        }
                    }
                }
            }
        }
        if (live && okn) {
            *reinterpret_cast<T*>(grad_x + s * N + n) = acc_x;
            if constexpr (PART) *reinterpret_cast<T*>(att_part + s * N + n) = acc_a;
        }
    }
}

template <int V>
hipError_t gatv2_score_w(int W, const int32_t* rowptr, const int32_t* colind, const float* xl, const float* xr, const float* att,
                         float* score, int M, int nnz, int H, int F, int epw, uint32_t magic, float slope, hipStream_t st) {
    const int nblk = (int)(((int64_t)nnz + kWaves * epw - 1) / (kWaves * epw));
    const int leaky = slope != 1.0f ? 1 : 0;
#define GESPMM_GV2(WW)                                                                                                               \
    case WW:                                                                                                                          \
        hipLaunchKernelGGL((gatv2_score_kernel<V, WW>), dim3(nblk), dim3(kThreads), 0, st, rowptr, colind, xl, xr, att, score, M, nnz, \
                           H, F, epw, magic, slope, leaky);                                                                           \
        return hipGetLastError();
    switch (W) {
        GESPMM_GV2(4)
        GESPMM_GV2(8)
        GESPMM_GV2(16)
        GESPMM_GV2(32)
        GESPMM_GV2(64)
    }
#undef GESPMM_GV2
    return hipErrorInvalidValue;
}

template <int V, bool PART>
hipError_t gatv2_score_backward_w(int W, const int32_t* ptr, const int32_t* ind, const int32_t* order, const float* grad_score,
                                  const float* x_seg, const float* x_ind, const float* att, float* grad_x, float* att_part, int S, int H,
                                  int F, float slope, hipStream_t st) {
    const int leaky = slope != 1.0f ? 1 : 0;
#define GESPMM_GV2B(WW)                                                                                                                 \
    case WW: {                                                                                                                           \
        const int per_block = kWaves * (64 / WW);                                                                                        \
        const int nblk = (int)(((int64_t)S + per_block - 1) / per_block);                                                                \
        hipLaunchKernelGGL((gatv2_score_backward_kernel<V, WW, PART>), dim3(nblk), dim3(kThreads), 0, st, ptr, ind, order, grad_score,   \
                           x_seg, x_ind, att, grad_x, att_part, S, H, F, slope, leaky);                                                  \
        return hipGetLastError();                                                                                                        \
    }
    switch (W) {
        GESPMM_GV2B(4)
        GESPMM_GV2B(8)
        GESPMM_GV2B(16)
        GESPMM_GV2B(32)
        GESPMM_GV2B(64)
    }
#undef GESPMM_GV2B
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_gatv2_score(const int32_t* rowptr, const int32_t* colind, const float* xl, const float* xr, const float* att,
                              float* score, int64_t M, int64_t nnz, int64_t H, int64_t F, float slope, const Gatv2ScoreLaunch& r,
                              hipStream_t st) {
    if (nnz < 1 || M < 1 || H < 1 || F < 1 || r.epw < 1 || r.epw > 256 || nnz > kSddmmMaxNnz / H || M > kSddmmMaxNnz / H ||
        M * H > kSddmmMaxNnz / F || (F % r.V) != 0)
        return hipErrorInvalidValue;
    const int m = (int)M, z = (int)nnz, h = (int)H, f = (int)F;
    if (r.V == 4) return gatv2_score_w<4>(r.W, rowptr, colind, xl, xr, att, score, m, z, h, f, r.epw, r.magic, slope, st);
    if (r.V == 2) return gatv2_score_w<2>(r.W, rowptr, colind, xl, xr, att, score, m, z, h, f, r.epw, r.magic, slope, st);
    if (r.V == 1) return gatv2_score_w<1>(r.W, rowptr, colind, xl, xr, att, score, m, z, h, f, r.epw, r.magic, slope, st);
    return hipErrorInvalidValue;
}

hipError_t launch_gatv2_score_backward(const int32_t* ptr, const int32_t* ind, const int32_t* order, const float* grad_score,
                                       const float* x_seg, const float* x_ind, const float* att, float* grad_x, float* att_part, int64_t S,
                                       int64_t H, int64_t F, int64_t nnz, float slope, bool vec4, hipStream_t st) {
    if (nnz < 1 || S < 1 || H < 1 || F < 1 || nnz > kSddmmMaxNnz / H || S > kSddmmMaxNnz / H || S * H > kSddmmMaxNnz / F ||
        (vec4 && (F % 4) != 0))
        return hipErrorInvalidValue;
    const int64_t N = H * F;
    const int64_t need = vec4 ? N / 4 : N;  // lanes that cover a row of N words
    int W = 4;
    while (W < 64 && W < need) W <<= 1;
    const int s = (int)S, h = (int)H, f = (int)F;
    if (vec4) {
        return att_part ? gatv2_score_backward_w<4, true>(W, ptr, ind, order, grad_score, x_seg, x_ind, att, grad_x, att_part, s, h, f, slope, st)
                        : gatv2_score_backward_w<4, false>(W, ptr, ind, order, grad_score, x_seg, x_ind, att, grad_x, att_part, s, h, f, slope, st);
    }
    return att_part ? gatv2_score_backward_w<1, true>(W, ptr, ind, order, grad_score, x_seg, x_ind, att, grad_x, att_part, s, h, f, slope, st)
                    : gatv2_score_backward_w<1, false>(W, ptr, ind, order, grad_score, x_seg, x_ind, att, grad_x, att_part, s, h, f, slope, st);
}

}  // namespace gespmm
