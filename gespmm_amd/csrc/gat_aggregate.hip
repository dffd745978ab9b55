// gat_aggregate.hip — the fused GAT aggregation (gat_aggregate.h): the multi-head batch-stream kernel of spmm_heads.hip with the H
// weights of a tile entry computed from el, er and the row statistics where that kernel loads them, its launch table, and the
// elementwise kernel that materialises the same weights for the composition route. A translation unit of its own: spmm_heads_kernel
// stays exactly what it is.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edge_dropout.h"
#include "gat_aggregate.h"
#include "spmm_device.h"

namespace gespmm {

// ----------------------------------------------------------------------------- the kernel
//
// Structure, row walk and store are spmm_heads_kernel's (see there; storage order only). What differs is where s_val comes from:
//   * lane k of a tile owns entry t0 + k. Its index ind[p] is loaded TWO tiles ahead (pc2), so that one tile ahead (fetch_terms) the
//     gathers that depend on it can be issued without waiting: per head el, er and the (m, s) pair of the entry's row — 4 words;
//   * the entry's segment is found in the wavefront's row pointers (s_ptr: at most kMaxRowsPerWave + 1, an upper-bound search in five
//     fixed steps, so runs of equal pointers — empty rows — are skipped). s_ptr is therefore published and the wavefront synchronised
//     BEFORE the first tile's terms are fetched;
//   * forward: the segment is the row (el, stats), the index the column (er). Transposed: the index is the row, the segment the column;
//   * publish_tile computes the weights and writes s_val[k H + h], the layout the row walk reads.
// A lane past the range's end keeps a valid index (0, or one it loaded earlier) and finds a valid segment (the search never leaves
// [0, nrows)), so every load is of a valid word; what it publishes is never read. No scratch, no atomics, no workspace.

//
// DROP (gespmm_gat_aggregate_dropout_f32; edge_dropout.h): the published weight becomes dropout(gat_weight(..)). The entry's (row, column)
// is known where its terms are fetched — forward (segment, index), transposed (index, segment): the same pair — so fetch_terms folds it
// into one word (the two mixes the heads share) and publish_tile spends one mix per head. The seed's two words are loaded once per
// wavefront, uniformly. Everything of it sits behind `if constexpr`: the DROP = false body is the kernel as it was.

template <int V, int S, int W, int U, bool TRANSPOSED, bool DROP>
__device__ __forceinline__ void gat_aggregate_body(const GatAggregateArgs& a, const EdgeDropout& drop) {
    constexpr int G = 64 / W;

    __shared__ uint32_t s_off[kWaves][kTile];
    __shared__ float s_val[kWaves][kTile * kHeadsMax];
    __shared__ int s_ptr[kWaves][kMaxRowsPerWave + 1];

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / W;
    const int l = lane % W;
    const int H = a.H;  // wave-uniform (kernel argument)
    uint32_t seed0 = 0, seed1 = 0, pent = 0;  // (DROP only) the seed; the entry's part of the mask's bits, fetched with its terms
    if constexpr (DROP) {
        seed0 = drop.seed[0];
        seed1 = drop.seed[1];
    }

    const int nitems = a.nblk * a.ntile;
    const int item = (a.flags & kFlagNoXcdRemap) ? (int)blockIdx.x : xcd_contiguous(blockIdx.x, nitems);
    int tile = 0, rb = item;
    if (a.ntile > 1) {
        tile = item % a.ntile;
        rb = item / a.ntile;
    }

    const int col0 = tile * (W * V * S) + l * V;
    bool colok[S];
    uint32_t cbytes[S];
    int head[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        colok[s] = (col0 + s * W * V) < a.N;
        // lanes/strips past N gather column 0 (valid, same line as lane 0) with the weights of head 0 and skip the store
        cbytes[s] = colok[s] ? (uint32_t)(col0 + s * W * V) * 4u : 0u;
        head[s] = colok[s] ? (col0 + s * W * V) / a.F : 0;
    }
    const char* Bbase = reinterpret_cast<const char*>(a.B);
    const uint32_t rowbytes = (uint32_t)a.N * 4u;
    const float2* stats = reinterpret_cast<const float2*>(a.stats);

    const int rpw = a.rpw;
    const int row_first = (rb * kWaves + wave) * rpw;
    if (row_first >= a.M) return;  // whole wavefront leaves together
    const int nrows = (a.M - row_first < rpw) ? a.M - row_first : rpw;
    // Row pointers of this wavefront's rows -> LDS (one coalesced load, rpw <= 32).
    const int rp = a.rowptr[row_first + (lane <= nrows ? lane : nrows)];
    if (lane <= kMaxRowsPerWave) s_ptr[wave][lane] = rp;
    const int wb = __builtin_amdgcn_readfirstlane(rp);
    const int we = __builtin_amdgcn_readlane(rp, nrows);
    wave_lds_sync();  // fetch_terms searches s_ptr

    // Tile stream state: `t0` = CSR position of the tile resident in LDS; pc / pel / per / pms belong to the tile after it, pc2 to the next.
    int pc = 0, pc2 = 0;
    float pel[kHeadsMax], per[kHeadsMax];
    float2 pms[kHeadsMax];
#pragma unroll
    for (int i = 0; i < kHeadsMax; ++i) {
        pel[i] = per[i] = 0.0f;
        pms[i] = make_float2(0.0f, 1.0f);
    }
    auto fetch_cols = [&](int base) {
        const int p = base + lane;
        if (p < we) pc2 = load_csr(a.colind + p);
    };
    auto fetch_terms = [&](int base) {  // `pc` holds the indices of the tile at `base`
        const int p = base + lane;
        int seg = 0;  // largest r < nrows with s_ptr[r] <= p (s_ptr[0] = wb <= p)
#pragma unroll
        for (int step = kMaxRowsPerWave / 2; step > 0; step >>= 1) {
            const int cand = seg + step;
            const int v = s_ptr[wave][cand < nrows ? cand : nrows];
            seg = (cand < nrows && v <= p) ? cand : seg;
        }
        const int rowi = (TRANSPOSED ? pc : row_first + seg) * H;  // (M H and K H words: 32-bit positions)
        const int coli = (TRANSPOSED ? row_first + seg : pc) * H;
        if constexpr (DROP)
            pent = edge_dropout_entry(seed0, (uint32_t)(TRANSPOSED ? pc : row_first + seg), (uint32_t)(TRANSPOSED ? row_first + seg : pc));
#pragma unroll
        for (int i = 0; i < kHeadsMax; ++i)
            if (i < H) {
                pel[i] = a.el[rowi + i];
                per[i] = a.er[coli + i];
                pms[i] = stats[rowi + i];
            }
    };
    auto publish_tile = [&]() {
        s_off[wave][lane] = (uint32_t)pc * rowbytes;
#pragma unroll
        for (int i = 0; i < kHeadsMax; ++i)
            if (i < H) {
                if constexpr (DROP)
                    s_val[wave][lane * H + i] = edge_dropout_apply(gat_weight(pel[i], per[i], pms[i], a.slope),
                                                                   edge_dropout_head(pent, seed1, (uint32_t)i), drop.threshold, drop.scale);
                else
                    s_val[wave][lane * H + i] = gat_weight(pel[i], per[i], pms[i], a.slope);
            }
    };
    auto advance = [&](int t0_) {  // after a publish: the registers move on by one tile
        pc = pc2;
        fetch_terms(t0_ + kTile);
        fetch_cols(t0_ + 2 * kTile);
    };

    fetch_cols(wb);
    pc = pc2;
    fetch_cols(wb + kTile);
    fetch_terms(wb);  // (the one dependent load of the task that nothing hides)

    int t0 = wb;
    publish_tile();
    advance(t0);
    wave_lds_sync();

    const bool nts = (a.flags & kFlagNtStore) != 0;
    for (int b = 0; b < nrows; b += G) {
        const int r = b + g;
        const bool rowok = r < nrows;
        int lb = 0, hb = 0;
        if (rowok) {
            lb = s_ptr[wave][r];
            hb = s_ptr[wave][r + 1];
        }
        const int be = __builtin_amdgcn_readfirstlane(s_ptr[wave][(b + G < nrows) ? b + G : nrows]);
        if constexpr (G == 1) {
            lb = __builtin_amdgcn_readfirstlane(lb);
            hb = __builtin_amdgcn_readfirstlane(hb);
        }

        float acc[S][V];
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int i = 0; i < V; ++i) acc[s][i] = 0.0f;

        for (;;) {
            const int tend = t0 + kTile;
            int k = (lb > t0 ? lb : t0) - t0;
            const int ke = (hb < tend ? hb : tend) - t0;
            // Full steps: U gathers issued back to back, no predicates.
            for (; k + U <= ke; k += U) {
                uint32_t off[U];
                float v[U][S];
                float bv[U][S][V];
#pragma unroll
                for (int j = 0; j < U; ++j) {
                    off[j] = s_off[wave][k + j];
#pragma unroll
                    for (int s = 0; s < S; ++s) v[j][s] = s_val[wave][(k + j) * H + head[s]];
                }
#pragma unroll
                for (int j = 0; j < U; ++j)
#pragma unroll
                    for (int s = 0; s < S; ++s) load_vec<V>(bv[j][s], Bbase + (uint32_t)(off[j] + cbytes[s]));
#pragma unroll
                for (int j = 0; j < U; ++j)
#pragma unroll
                    for (int s = 0; s < S; ++s)
#pragma unroll
                        for (int i = 0; i < V; ++i) acc[s][i] = __builtin_fmaf(v[j][s], bv[j][s][i], acc[s][i]);
            }
            // Tail (1..U-1 entries): ONE predicated group; LDS reads first (clamped slot: always inside the tile), then the gathers.
            const int rem = ke - k;
            if (rem > 0) {
                uint32_t off[U - 1];
                float v[U - 1][S];
                float bv[U - 1][S][V];
#pragma unroll
                for (int j = 0; j < U - 1; ++j) {
                    const int kj = k + ((j < rem) ? j : rem - 1);
                    off[j] = s_off[wave][kj];
#pragma unroll
                    for (int s = 0; s < S; ++s) v[j][s] = s_val[wave][kj * H + head[s]];
                }
#pragma unroll
                for (int j = 0; j < U - 1; ++j) {
                    if (j < rem) {
#pragma unroll
                        for (int s = 0; s < S; ++s) load_vec<V>(bv[j][s], Bbase + (uint32_t)(off[j] + cbytes[s]));
                    }
                }
#pragma unroll
                for (int j = 0; j < U - 1; ++j) {
                    if (j < rem) {
#pragma unroll
                        for (int s = 0; s < S; ++s)
#pragma unroll
                            for (int i = 0; i < V; ++i) acc[s][i] = __builtin_fmaf(v[j][s], bv[j][s][i], acc[s][i]);
                    }
                }
            }
            if (be <= tend) break;  // every row of this batch ends inside the resident tile
            wave_lds_sync();        // all reads of the old tile are issued before it is overwritten
            t0 = tend;
            publish_tile();
            advance(t0);
            wave_lds_sync();
        }

        if (rowok) {
            float* Crow = a.C + (size_t)(row_first + r) * (size_t)a.N + col0;
#pragma unroll
            for (int s = 0; s < S; ++s)
                if (colok[s]) {
                    if (nts) store_vec<V, true>(Crow + s * (W * V), acc[s]);
                    else store_vec<V, false>(Crow + s * (W * V), acc[s]);
                }
        }
    }
}

template <int V, int S, int W, int U, bool TRANSPOSED>
__global__ __launch_bounds__(kThreads) void gat_aggregate_kernel(GatAggregateArgs a) {
    gat_aggregate_body<V, S, W, U, TRANSPOSED, false>(a, EdgeDropout{});
}

template <int V, int S, int W, int U, bool TRANSPOSED>
__global__ __launch_bounds__(kThreads) void gat_aggregate_dropout_kernel(GatAggregateArgs a, EdgeDropout drop) {
    gat_aggregate_body<V, S, W, U, TRANSPOSED, true>(a, drop);
}

// ----------------------------------------------------------------------------- launch table (launch_heads of spmm_heads.hip, storage order)

template <int V, int S, int W>
static hipError_t launch_gat(const GatAggregateArgs& a, int rpw, bool transposed, const EdgeDropout* drop, hipStream_t st) {
    constexpr int G = 64 / W;
    constexpr int U = (V * S >= 8) ? 4 : 8;
    GatAggregateArgs args = a;
    if (rpw < G) rpw = G;
    if (rpw > kMaxRowsPerWave) rpw = kMaxRowsPerWave;
    rpw = rpw / G * G;
    args.ntile = (a.N + W * V * S - 1) / (W * V * S);
    while (rpw < kMaxRowsPerWave && (((int64_t)a.M + kWaves * rpw - 1) / (kWaves * rpw)) * args.ntile > kMaxGridBlocks) {
        rpw *= 2;  // (the grid must fit 2^32 threads: tasks grow, never past the kernel's row-pointer staging)
        if (rpw > kMaxRowsPerWave) rpw = kMaxRowsPerWave;
        rpw = rpw / G * G;
    }
    args.rpw = rpw;
    args.nblk = (int)(((int64_t)a.M + kWaves * rpw - 1) / (kWaves * rpw));
    const int64_t nitems = (int64_t)args.nblk * args.ntile;
    if (nitems <= 0) return hipSuccess;
    if (nitems > kMaxGridBlocks) return hipErrorInvalidConfiguration;
    if (drop) {
        if (transposed)
            hipLaunchKernelGGL((gat_aggregate_dropout_kernel<V, S, W, U, true>), dim3((unsigned)nitems), dim3(kThreads), 0, st, args, *drop);
        else
            hipLaunchKernelGGL((gat_aggregate_dropout_kernel<V, S, W, U, false>), dim3((unsigned)nitems), dim3(kThreads), 0, st, args, *drop);
        return hipGetLastError();
    }
    if (transposed) hipLaunchKernelGGL((gat_aggregate_kernel<V, S, W, U, true>), dim3((unsigned)nitems), dim3(kThreads), 0, st, args);
    else hipLaunchKernelGGL((gat_aggregate_kernel<V, S, W, U, false>), dim3((unsigned)nitems), dim3(kThreads), 0, st, args);
    return hipGetLastError();
}

hipError_t launch_gat_aggregate(const GatAggregateArgs& a, const Geometry& g, bool transposed, const EdgeDropout* drop, hipStream_t st) {
    if (drop && !drop->seed) return hipErrorInvalidValue;
    if (a.H < 1 || a.H > kHeadsMax || a.F < 1 || a.N != a.H * a.F || a.F % g.vec != 0) return hipErrorInvalidValue;
    if (!a.rowptr || !a.colind || !a.B || !a.C || !a.el || !a.er || !a.stats) return hipErrorInvalidValue;
    if (!heads_geometry_served(g, false)) return hipErrorInvalidValue;
#define GESPMM_GAT(V_, S_, W_) \
    if (g.vec == V_ && g.strips == S_ && g.group == W_) return launch_gat<V_, S_, W_>(a, g.rows_per_wave, transposed, drop, st);
    GESPMM_GAT(1, 1, 4)
    GESPMM_GAT(1, 1, 8)
    GESPMM_GAT(1, 1, 16)
    GESPMM_GAT(1, 1, 32)
    GESPMM_GAT(1, 1, 64)
    GESPMM_GAT(4, 1, 32)
    GESPMM_GAT(4, 1, 64)
    GESPMM_GAT(4, 2, 64)
    GESPMM_GAT(2, 1, 64)
    GESPMM_GAT(2, 2, 64)
    GESPMM_GAT(1, 2, 64)
#undef GESPMM_GAT
    return hipErrorInvalidValue;
}

// ----------------------------------------------------------------------------- composition route: the weights as an array, grid-stride

template <bool TRANSPOSED>
__global__ __launch_bounds__(256) void gat_weights_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ ind,
                                                          const float* __restrict__ el, const float* __restrict__ er,
                                                          const float* __restrict__ stats, float* __restrict__ w, int S, int H, int64_t n,
                                                          float slope) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int p = (int)(i / H), h = (int)(i - (int64_t)p * H);
        const int seg = row_of_entry(ptr, S, p), j = ind[p];
        const int r = TRANSPOSED ? j : seg, c = TRANSPOSED ? seg : j;
        w[i] = gat_weight(el[r * H + h], er[c * H + h], reinterpret_cast<const float2*>(stats)[r * H + h], slope);
    }
}

hipError_t launch_gat_weights(const int32_t* ptr, const int32_t* ind, const float* el, const float* er, const float* stats, float* w,
                              int64_t S, int64_t H, int64_t nnz, float slope, bool transposed, hipStream_t st) {
    if (nnz <= 0 || H <= 0) return hipSuccess;
    if (S < 1 || nnz * H >= (1ll << 31)) return hipErrorInvalidValue;
    const int64_t n = nnz * H;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;  // a few workgroups per CU, grid-stride beyond
    if (transposed)
        hipLaunchKernelGGL(gat_weights_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, ptr, ind, el, er, stats, w, (int)S, (int)H, n, slope);
    else
        hipLaunchKernelGGL(gat_weights_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, ptr, ind, el, er, stats, w, (int)S, (int)H, n, slope);
    return hipGetLastError();
}

}  // namespace gespmm
