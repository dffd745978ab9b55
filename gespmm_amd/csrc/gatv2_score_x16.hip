// gatv2_score_x16.hip — the GATv2 edge score and its gradients on 16-bit node operands (IEEE fp16 / bfloat16 xl, xr, x_seg, x_ind and
// grad_x of one type; att, grad_score, score and att_part stay fp32; gfx950). Contract, pinned orders and safety rules: gatv2_score.h.
//
//     score[p H + h] = sum_f att[h, f] * leaky(fl32(widen(xl[row(p), h, f]) + widen(xr[col(p), h, f])))      (CSR entry order, head-minor)
//
// The two kernels of gatv2_score.hip with a lane's vector counted in ELEMENTS: V elements of xl / xr are V / 2 32-bit words (dwordx4,
// dwordx2, dword loads for V = 8, 4, 2; V = 1 is one ushort), the V floats of att at the same element positions are one or two loads of
// at most 16 bytes. Every element is widened — exactly, subnormals included (widen_x16, spmm_device.h) — at its use; the arithmetic is
// the fp32 kernels': one fp32 add, the branch t >= 0, one fmaf per element. No packed-fp16 arithmetic and no dot2: they round
// differently. grad_x is rounded ONCE, at the store (narrow_x16).

#include "gatv2_score.h"

#include "spmm_device.h"
#include "spmm_kernels.h"

namespace gespmm {

namespace {

// V 16-bit elements as (V + 1) / 2 words, the lower-addressed element of a word in its low half (V = 1: the low half alone).
template <int V> struct Gx16Words { static constexpr int n = (V + 1) / 2; uint32_t w[n]; };

template <int V> __device__ __forceinline__ Gx16Words<V> gx16_load(const uint16_t* __restrict__ p) {
    Gx16Words<V> r;
    if constexpr (V == 1) {
        r.w[0] = *p;
    } else if constexpr (V == 2) {
        r.w[0] = *reinterpret_cast<const uint32_t*>(p);
    } else if constexpr (V == 4) {
        const uint2 t = *reinterpret_cast<const uint2*>(p);
        r.w[0] = t.x, r.w[1] = t.y;
    } else {
        const uint4 t = *reinterpret_cast<const uint4*>(p);
        r.w[0] = t.x, r.w[1] = t.y, r.w[2] = t.z, r.w[3] = t.w;
    }
    return r;
}

template <int V> __device__ __forceinline__ void gx16_store(uint16_t* __restrict__ p, const Gx16Words<V>& r) {
    if constexpr (V == 1) *p = (uint16_t)r.w[0];
    else if constexpr (V == 2) *reinterpret_cast<uint32_t*>(p) = r.w[0];
    else if constexpr (V == 4) *reinterpret_cast<uint2*>(p) = make_uint2(r.w[0], r.w[1]);
    else *reinterpret_cast<uint4*>(p) = make_uint4(r.w[0], r.w[1], r.w[2], r.w[3]);
}

// element i of the vector, widened exactly
template <int DT, int V> __device__ __forceinline__ float gx16_get(const Gx16Words<V>& r, int i) {
    float lo, hi;
    widen_x16<DT>(__uint_as_float(r.w[i >> 1]), lo, hi);
    return (i & 1) ? hi : lo;
}

// V floats of att / att_part at the element positions of a 16-bit vector: loads and stores of at most 16 bytes
template <int V> struct Gx16Floats { float f[V]; };

template <int V> __device__ __forceinline__ Gx16Floats<V> gx16_load_f32(const float* __restrict__ p) {
    Gx16Floats<V> r;
    if constexpr (V == 1) {
        r.f[0] = *p;
    } else if constexpr (V == 2) {
        const float2 t = *reinterpret_cast<const float2*>(p);
        r.f[0] = t.x, r.f[1] = t.y;
    } else {
#pragma unroll
        for (int k = 0; k < V / 4; ++k) {
            const float4 t = reinterpret_cast<const float4*>(p)[k];
            r.f[4 * k] = t.x, r.f[4 * k + 1] = t.y, r.f[4 * k + 2] = t.z, r.f[4 * k + 3] = t.w;
        }
    }
    return r;
}

template <int V> __device__ __forceinline__ void gx16_store_f32(float* __restrict__ p, const Gx16Floats<V>& r) {
    if constexpr (V == 1) {
        *p = r.f[0];
    } else if constexpr (V == 2) {
        *reinterpret_cast<float2*>(p) = make_float2(r.f[0], r.f[1]);
    } else {
#pragma unroll
        for (int k = 0; k < V / 4; ++k)
            reinterpret_cast<float4*>(p)[k] = make_float4(r.f[4 * k], r.f[4 * k + 1], r.f[4 * k + 2], r.f[4 * k + 3]);
    }
}

// leaky(t) = t >= 0 ? t : slope * t. `leaky` is false for slope == 1: no multiply.
__device__ __forceinline__ float gx16_leaky(float t, float slope, bool leaky) { return (leaky && !(t >= 0.0f)) ? slope * t : t; }

// Row that owns CSR position e: largest r with rowptr[r] <= e (empty rows skipped).
__device__ __forceinline__ int gx16_row_of_entry(const int32_t* __restrict__ rowptr, int M, int e) {
    int lo = 0, hi = M;  // invariant: rowptr[lo] <= e < rowptr[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rowptr[mid] <= e) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The same for a wavefront-uniform e, all 64 lanes probing at once: every round cuts [lo, hi) into 64 pieces.
__device__ __forceinline__ int gx16_row_of_entry_wave(const int32_t* __restrict__ rowptr, int M, int e, int lane) {
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

// ---- forward: gatv2_score_kernel (gatv2_score.hip) on 16-bit xl / xr. UE pairs per lane group and step: 4, as in fp32, up to V = 4
// (a pair holds 2 (V / 2) + V registers of loads: 32 at V = 4, what the fp32 kernel holds at its V = 4 is 48); at V = 8 a pair is 16
// registers and UE = 4 would hold 64 — with addresses and sums past the 64 registers that let eight wavefronts share a SIMD — so two.
template <int V> constexpr int gx16_ue() { return V == 8 ? 2 : 4; }

template <int DT, int V, int W>
__global__ __launch_bounds__(kThreads) void gatv2_score_x16_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                                    const uint16_t* __restrict__ xl, const uint16_t* __restrict__ xr,
                                                                    const float* __restrict__ att, float* __restrict__ score, int M,
                                                                    int nnz, int H, int F, int epw, uint32_t magic, float slope,
                                                                    int leaky_i) {
    constexpr int G = 64 / W;
    constexpr int EPW = 256;  // most entries a wavefront owns (epw <= EPW): one row search per epw entries, their ids in LDS
    constexpr int UE = gx16_ue<V>();
    const bool leaky = leaky_i != 0;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / W;
    const int l = lane % W;

    // ---- the wavefront's entries [e_lo, e_hi): ONE wavefront-wide search for the row of the first entry, the epw + 2 row pointers from
    // there in LDS, every lane resolves one entry (the whole-array search when more than epw empty rows fall into the window).
    __shared__ int s_rp[kWaves][EPW + 2];
    __shared__ int s_row[kWaves][EPW];
    __shared__ int s_col[kWaves][EPW];
    const int e_lo = (blockIdx.x * kWaves + wave) * epw;
    if (e_lo >= nnz) return;  // whole wavefront
    const int e_hi = (e_lo + epw < nnz) ? e_lo + epw : nnz;
    const int r0 = gx16_row_of_entry_wave(rowptr, M, e_lo, lane);
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
                lo = gx16_row_of_entry(rowptr, M, e) - r0;
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
    const int ld = H * F;                        // ELEMENTS between two rows of xl / xr (M H F, K H F <= kSddmmMaxNnz: 32-bit positions)
    const int nT = (F + W * V - 1) / (W * V);    // vectors per lane and slice: wave-uniform
    for (int rb = 0; rb < q_hi - q_lo; rb += G * UE) {
        const int qbase = q_lo + rb + g * UE;
        // Pair q -> its three head slices. A pair past the wavefront's end takes the last valid pair (re-read, dropped at the store).
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
            Gx16Words<V> x[UE], y[UE];  // all loads of the group's UE pairs are requested before any is used
            Gx16Floats<V> a[UE];
#pragma unroll
            for (int u = 0; u < UE; ++u) {
                x[u] = gx16_load<V>(xl + o1[u] + jj);
                y[u] = gx16_load<V>(xr + o2[u] + jj);
                a[u] = gx16_load_f32<V>(att + o3[u] + jj);
            }
#pragma unroll
            for (int u = 0; u < UE; ++u) {
#pragma unroll
                for (int i = 0; i < V; ++i) {  // a lane past the slice contributes fmaf(0, 0, 0)
                    const float xi = in ? gx16_get<DT, V>(x[u], i) : 0.0f;
                    const float yi = in ? gx16_get<DT, V>(y[u], i) : 0.0f;
                    const float ai = in ? a[u].f[i] : 0.0f;
                    part[u] = __builtin_fmaf(ai, gx16_leaky(xi + yi, slope, leaky), part[u]);
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

// ---- backward: gatv2_score_backward_kernel (gatv2_score.hip) on 16-bit x_seg / x_ind / grad_x: a group of W lanes walks one segment at
// width N = H F; one fmaf chain per output word, in segment order; the sum is narrowed once at the store. UG = 4 gathers in flight as in
// fp32: a gathered vector is V / 2 registers — at V = 8 the four of an fp32 V = 4 vector.
template <int DT, int V, int W, bool PART>
__global__ __launch_bounds__(kThreads) void gatv2_score_backward_x16_kernel(
    const int32_t* __restrict__ ptr, const int32_t* __restrict__ ind, const int32_t* __restrict__ order,
    const float* __restrict__ grad_score, const uint16_t* __restrict__ x_seg, const uint16_t* __restrict__ x_ind,
    const float* __restrict__ att, uint16_t* __restrict__ grad_x, float* __restrict__ att_part, int S, int H, int F, float slope,
    int leaky_i) {
    constexpr int G = 64 / W;
    constexpr int UG = 4;  // gathers of x_ind rows in flight per lane (W is a multiple of 4)
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
    const int N = H * F;  // (S H F, T H F <= kSddmmMaxNnz: 32-bit element positions)
    for (int n0 = 0; n0 < N; n0 += W * V) {
        const int n = n0 + l * V;
        const bool okn = n < N;  // (V divides F, hence N: a lane's vector is inside the row or past it, whole, and inside ONE head)
        const int nn = okn ? n : 0;
        const int h = nn / F;
        const Gx16Words<V> xs = gx16_load<V>(x_seg + sc * N + nn);
        const Gx16Floats<V> a = gx16_load_f32<V>(att + nn);
        Gx16Floats<V> as = a;  // fl(att * slope): the factor of an entry on the negative side
        if (leaky) {
#pragma unroll
            for (int i = 0; i < V; ++i) as.f[i] = a.f[i] * slope;
        }
        Gx16Floats<V> acc_x, acc_a;
#pragma unroll
        for (int i = 0; i < V; ++i) acc_x.f[i] = 0.0f, acc_a.f[i] = 0.0f;
        for (int p0 = 0; p0 < dmax; p0 += W) {
            // W entries per group, coalesced, then broadcast. A lane past its segment re-reads the segment's first entry (entry 0 where
            // the segment is empty: nnz >= 1); what it gathers is dropped by the select below.
            const int pe = p0 + l;
            const int e = pe < d ? lo + pe : (d > 0 ? lo : 0);
            const int c = ind[e];
            const int q = order ? order[e] : e;
            const int kmax = (dmax - p0 < W) ? dmax - p0 : W;
            for (int k0 = 0; k0 < kmax; k0 += UG) {
                Gx16Words<V> xv[UG];
                float gv[UG];
#pragma unroll
                for (int u = 0; u < UG; ++u) {
                    const int ck = __shfl(c, k0 + u, W);
                    const int qk = __shfl(q, k0 + u, W);
                    xv[u] = gx16_load<V>(x_ind + ck * N + nn);
                    gv[u] = grad_score[qk * H + h];
                }
#pragma unroll
                for (int u = 0; u < UG; ++u) {
                    const bool valid = p0 + k0 + u < d;
#pragma unroll
                    for (int i = 0; i < V; ++i) {
                        const float t = gx16_get<DT, V>(xs, i) + gx16_get<DT, V>(xv[u], i);
                        const bool neg = leaky && !(t >= 0.0f);
                        const float m = neg ? as.f[i] : a.f[i];
                        const float ax = __builtin_fmaf(gv[u], m, acc_x.f[i]);
                        acc_x.f[i] = valid ? ax : acc_x.f[i];
                        if constexpr (PART) {
                            const float aa = __builtin_fmaf(gv[u], neg ? slope * t : t, acc_a.f[i]);
                            acc_a.f[i] = valid ? aa : acc_a.f[i];
                        }
                    }
                    // one gathered vector at a time: the V comparisons of a vector are lane masks in scalar registers, and a scheduler
                    // free to hoist those of all UG vectors runs out of them at V = 8
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        if (live && okn) {
            Gx16Words<V> out;  // ONE rounding per element, to nearest even
#pragma unroll
            for (int i = 0; i < Gx16Words<V>::n; ++i) {
                out.w[i] = narrow_x16<DT>(acc_x.f[2 * i]);
                if constexpr (V > 1) out.w[i] |= narrow_x16<DT>(acc_x.f[2 * i + 1]) << 16;
            }
            gx16_store<V>(grad_x + s * N + n, out);
            if constexpr (PART) gx16_store_f32<V>(att_part + s * N + n, acc_a);
        }
    }
}

template <int DT, int V>
hipError_t gatv2_score_x16_w(int W, const int32_t* rowptr, const int32_t* colind, const uint16_t* xl, const uint16_t* xr, const float* att,
                             float* score, int M, int nnz, int H, int F, int epw, uint32_t magic, float slope, hipStream_t st) {
    const int nblk = (int)(((int64_t)nnz + kWaves * epw - 1) / (kWaves * epw));
    const int leaky = slope != 1.0f ? 1 : 0;
#define GESPMM_GX16(WW)                                                                                                                  \
    case WW:                                                                                                                              \
        hipLaunchKernelGGL((gatv2_score_x16_kernel<DT, V, WW>), dim3(nblk), dim3(kThreads), 0, st, rowptr, colind, xl, xr, att, score, M,  \
                           nnz, H, F, epw, magic, slope, leaky);                                                                          \
        return hipGetLastError();
    switch (W) {
        GESPMM_GX16(4)
        GESPMM_GX16(8)
        GESPMM_GX16(16)
        GESPMM_GX16(32)
        GESPMM_GX16(64)
    }
#undef GESPMM_GX16
    return hipErrorInvalidValue;
}

template <int DT, int V, bool PART>
hipError_t gatv2_score_backward_x16_w(int W, const int32_t* ptr, const int32_t* ind, const int32_t* order, const float* grad_score,
                                      const uint16_t* x_seg, const uint16_t* x_ind, const float* att, uint16_t* grad_x, float* att_part,
                                      int S, int H, int F, float slope, hipStream_t st) {
    const int leaky = slope != 1.0f ? 1 : 0;
#define GESPMM_GX16B(WW)                                                                                                                 \
    case WW: {                                                                                                                            \
        const int per_block = kWaves * (64 / WW);                                                                                         \
        const int nblk = (int)(((int64_t)S + per_block - 1) / per_block);                                                                 \
        hipLaunchKernelGGL((gatv2_score_backward_x16_kernel<DT, V, WW, PART>), dim3(nblk), dim3(kThreads), 0, st, ptr, ind, order,        \
                           grad_score, x_seg, x_ind, att, grad_x, att_part, S, H, F, slope, leaky);                                       \
        return hipGetLastError();                                                                                                         \
    }
    switch (W) {
        GESPMM_GX16B(4)
        GESPMM_GX16B(8)
        GESPMM_GX16B(16)
        GESPMM_GX16B(32)
        GESPMM_GX16B(64)
    }
#undef GESPMM_GX16B
    return hipErrorInvalidValue;
}

template <int DT>
hipError_t gatv2_score_x16_dt(const int32_t* rowptr, const int32_t* colind, const uint16_t* xl, const uint16_t* xr, const float* att,
                              float* score, int m, int z, int h, int f, const Gatv2ScoreLaunch& r, float slope, hipStream_t st) {
    if (r.V == 8) return gatv2_score_x16_w<DT, 8>(r.W, rowptr, colind, xl, xr, att, score, m, z, h, f, r.epw, r.magic, slope, st);
    if (r.V == 4) return gatv2_score_x16_w<DT, 4>(r.W, rowptr, colind, xl, xr, att, score, m, z, h, f, r.epw, r.magic, slope, st);
    if (r.V == 2) return gatv2_score_x16_w<DT, 2>(r.W, rowptr, colind, xl, xr, att, score, m, z, h, f, r.epw, r.magic, slope, st);
    if (r.V == 1) return gatv2_score_x16_w<DT, 1>(r.W, rowptr, colind, xl, xr, att, score, m, z, h, f, r.epw, r.magic, slope, st);
    return hipErrorInvalidValue;
}

template <int DT, int V>
hipError_t gatv2_score_backward_x16_v(int W, const int32_t* ptr, const int32_t* ind, const int32_t* order, const float* grad_score,
                                      const uint16_t* x_seg, const uint16_t* x_ind, const float* att, uint16_t* grad_x, float* att_part,
                                      int s, int h, int f, float slope, hipStream_t st) {
    return att_part ? gatv2_score_backward_x16_w<DT, V, true>(W, ptr, ind, order, grad_score, x_seg, x_ind, att, grad_x, att_part, s, h, f,
                                                              slope, st)
                    : gatv2_score_backward_x16_w<DT, V, false>(W, ptr, ind, order, grad_score, x_seg, x_ind, att, grad_x, att_part, s, h, f,
                                                               slope, st);
}

template <int DT>
hipError_t gatv2_score_backward_x16_dt(int V, int W, const int32_t* ptr, const int32_t* ind, const int32_t* order, const float* grad_score,
                                       const uint16_t* x_seg, const uint16_t* x_ind, const float* att, uint16_t* grad_x, float* att_part,
                                       int s, int h, int f, float slope, hipStream_t st) {
    if (V == 8) return gatv2_score_backward_x16_v<DT, 8>(W, ptr, ind, order, grad_score, x_seg, x_ind, att, grad_x, att_part, s, h, f, slope, st);
    if (V == 4) return gatv2_score_backward_x16_v<DT, 4>(W, ptr, ind, order, grad_score, x_seg, x_ind, att, grad_x, att_part, s, h, f, slope, st);
    if (V == 2) return gatv2_score_backward_x16_v<DT, 2>(W, ptr, ind, order, grad_score, x_seg, x_ind, att, grad_x, att_part, s, h, f, slope, st);
    if (V == 1) return gatv2_score_backward_x16_v<DT, 1>(W, ptr, ind, order, grad_score, x_seg, x_ind, att, grad_x, att_part, s, h, f, slope, st);
    return hipErrorInvalidValue;
}

}  // namespace

int gatv2_score_x16_vec(int64_t F, int x_align, int f_align) {
    int V = 8;
    while (V > 1 && ((F % V) != 0 || (x_align % (2 * V)) != 0 || (f_align % (4 * V < 16 ? 4 * V : 16)) != 0)) V >>= 1;
    return V;
}

hipError_t launch_gatv2_score_x16(const int32_t* rowptr, const int32_t* colind, const void* xl, const void* xr, const float* att,
                                  float* score, int dtype, int64_t M, int64_t nnz, int64_t H, int64_t F, float slope,
                                  const Gatv2ScoreLaunch& r, hipStream_t st) {
    if (nnz < 1 || M < 1 || H < 1 || F < 1 || r.epw < 1 || r.epw > 256 || nnz > kSddmmMaxNnz / H || M > kSddmmMaxNnz / H ||
        M * H > kSddmmMaxNnz / F || r.V < 1 || (F % r.V) != 0)
        return hipErrorInvalidValue;
    const int m = (int)M, z = (int)nnz, h = (int)H, f = (int)F;
    const uint16_t* l16 = static_cast<const uint16_t*>(xl);
    const uint16_t* r16 = static_cast<const uint16_t*>(xr);
    if (dtype == kX16F16) return gatv2_score_x16_dt<kX16F16>(rowptr, colind, l16, r16, att, score, m, z, h, f, r, slope, st);
    if (dtype == kX16Bf16) return gatv2_score_x16_dt<kX16Bf16>(rowptr, colind, l16, r16, att, score, m, z, h, f, r, slope, st);
    return hipErrorInvalidValue;
}

hipError_t launch_gatv2_score_backward_x16(const int32_t* ptr, const int32_t* ind, const int32_t* order, const float* grad_score,
                                           const void* x_seg, const void* x_ind, const float* att, void* grad_x, float* att_part, int dtype,
                                           int64_t S, int64_t H, int64_t F, int64_t nnz, float slope, int V, hipStream_t st) {
    if (nnz < 1 || S < 1 || H < 1 || F < 1 || nnz > kSddmmMaxNnz / H || S > kSddmmMaxNnz / H || S * H > kSddmmMaxNnz / F || V < 1 ||
        (F % V) != 0)
        return hipErrorInvalidValue;
    const int64_t need = H * F / V;  // lanes that cover a row of N elements
    int W = 4;
    while (W < 64 && W < need) W <<= 1;
    const int s = (int)S, h = (int)H, f = (int)F;
    const uint16_t* xs = static_cast<const uint16_t*>(x_seg);
    const uint16_t* xi = static_cast<const uint16_t*>(x_ind);
    uint16_t* gx = static_cast<uint16_t*>(grad_x);
    if (dtype == kX16F16)
        return gatv2_score_backward_x16_dt<kX16F16>(V, W, ptr, ind, order, grad_score, xs, xi, att, gx, att_part, s, h, f, slope, st);
    if (dtype == kX16Bf16)
        return gatv2_score_backward_x16_dt<kX16Bf16>(V, W, ptr, ind, order, grad_score, xs, xi, att, gx, att_part, s, h, f, slope, st);
    return hipErrorInvalidValue;
}

}  // namespace gespmm
