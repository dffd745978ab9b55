// spmm_heads_kernel.h — the body of the multi-head batch-stream kernel as a template on the ELEMENT TYPE of B and C, and the grid of its
// launch. Included by spmm_heads.hip (DT = 0: fp32, the kernels of gespmm_csr_spmm_heads_f32 — their instruction streams are what they
// were when the body stood in that file) and by spmm_heads_x16.hip (DT = kX16F16 / kX16Bf16: gespmm_csr_spmm_heads_x16).
//
// The structure is spmm_stream_kernel's (see there): a wavefront owns `rpw` consecutive rows = one contiguous CSR range, row pointers in
// LDS by one coalesced load, the range streams through a 64-entry LDS tile with the next tile prefetched in registers, rows are walked
// G = 64 / W at a time, U gathers back to back and one predicated tail group. What differs:
//   * the tile stages 64 H weights, not 64: the weights of tile [t0, t0 + 64) are the contiguous range val[t0 H, (t0 + 64) H), loaded
//     fully coalesced (word i * 64 + lane of the range, i < H) and kept in registers one tile ahead like the columns;
//   * a lane's strip s covers V contiguous columns of ONE head (V divides F): head[s] = column / F, computed once before the row loop,
//     and the FMA operand of tile entry k is s_val[k H + head[s]] — lanes of one head read one address (broadcast);
//   * sum reducer, valued, 32-bit offsets, strict CSR order only (no long-row registration).
// H is a runtime value <= kHeadsMax; every loop over heads is unrolled to kHeadsMax under a wave-uniform `i < H`.
// LDS per workgroup: s_off 1 KB + s_val 8 KB + s_ptr 528 B (+ s_perm 512 B in plan mode) — about 10 KB, no limit on occupancy.
//
// 16-bit elements (DT != 0): the kernel works in 32-bit WORDS, the way the 16-bit streaming kernels do (spmm_kernels.h: HalfSpmmArgs).
// a.B / a.C are arrays of words, a.N the words of a row (H F / 2), a.F the words of a head (F / 2), V words per lane and strip; every
// address, the lane geometry and the staged weights are the fp32 kernel's at half the width. A gathered word widens — exactly — into
// two fp32 values that share the staged weight of their head (2 V S accumulators, one fmaf chain each in CSR order), and the row-end
// store rounds each sum once, to nearest even, and packs the pairs (widen_x16 / narrow_x16 of spmm_device.h).
//
// ORDERED (spmm_heads_order.hip; storage order only): the weights of tile entry p are row a.order[p] of val, not row p. Only the tile
// staging differs — the lane that owns entry p = base + lane loads order[p] (coalesced, like colind) ONE TILE FURTHER AHEAD than the
// weights, so the dependent gather of the H words val[order[p] H ..] (the widest load H and the alignment of val allow: 16 bytes for
// H = 4 / 8, 8 bytes for H = 2 / 4 / 8, dwords otherwise; wave-uniform) is issued one tile ahead like the unordered weights, with its
// address already in a register. The lane publishes its H words at s_val[lane H + head], where the row loop reads them. Row loop,
// gathers of B, accumulators and stores are the unordered kernel's: the bits are those of the unordered kernel on the permuted copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spmm_device.h"
#include "spmm_heads.h"

namespace gespmm {

template <int DT, int V, int S, int W, int U, bool PLANNED, bool ORDERED = false>
__global__ __launch_bounds__(kThreads) void spmm_heads_kernel_t(HeadsArgsOf<ORDERED> a) {
    static_assert(!(ORDERED && PLANNED), "a plan permutes its weights through the order in the copy it already makes");
    constexpr int G = 64 / W;
    constexpr int E = (DT != 0) ? 2 : 1;  // fp32 sums per gathered word

    __shared__ uint32_t s_off[kWaves][kTile];
    __shared__ alignas(ORDERED ? 16 : alignof(float)) float s_val[kWaves][kTile * kHeadsMax];  // (ORDERED publishes 16-byte slots)
    __shared__ int s_ptr[kWaves][kMaxRowsPerWave + 1];
    __shared__ int s_perm[PLANNED ? kWaves : 1][PLANNED ? kMaxRowsPerWave : 1];

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / W;
    const int l = lane % W;
    const int H = a.H;  // wave-uniform (kernel argument)

    const int nitems = a.nblk * a.ntile;
    const int item = (a.flags & kFlagNoXcdRemap) ? (int)blockIdx.x : xcd_contiguous(blockIdx.x, nitems);
    int tile = 0, rb = item;
    if (a.ntile > 1) {
        tile = item % a.ntile;
        rb = item / a.ntile;
    }
    int row_first, nrows, wb, we;  // wave-uniform
    int rp_plan = 0, pm_plan = 0;

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

    // Tile stream state: `t0` = CSR position of the tile resident in LDS.
    int pc = 0;
    float pv[kHeadsMax];
#pragma unroll
    for (int i = 0; i < kHeadsMax; ++i) pv[i] = 0.0f;
    int po = 0;  // ORDERED: order[] of the entry this lane owns in the tile AFTER the one whose weights are fetched next
    int vw = 1;  // ORDERED: words per weight load (wave-uniform)
    if constexpr (ORDERED) {
        const uint32_t va = (uint32_t)reinterpret_cast<uintptr_t>(a.val);
        if ((H == 4 || H == 8) && va % 16u == 0) vw = 4;
        else if ((H == 2 || H == 4 || H == 8) && va % 8u == 0) vw = 2;
    }
    auto fetch_tile_regs = [&](int base) {
        const int p = base + lane;
        if (p < we) pc = load_csr(a.colind + p);
        if constexpr (ORDERED) {
            // `po` is order[p], loaded when the previous tile was fetched (or before the first): the H words of that row of val now,
            // order[p + 64] for the next call. Neither array is read at or past `we`.
            if (p < we) {
                const float* src = a.val + (uint32_t)po * (uint32_t)H;  // (nnz H < 2^31: no wrap)
                if (vw == 4) {
#pragma unroll
                    for (int j = 0; j < kHeadsMax / 4; ++j)
                        if (j * 4 < H) {
                            const float4 w = *reinterpret_cast<const float4*>(src + j * 4);
                            pv[j * 4] = w.x, pv[j * 4 + 1] = w.y, pv[j * 4 + 2] = w.z, pv[j * 4 + 3] = w.w;
                        }
                } else if (vw == 2) {
#pragma unroll
                    for (int j = 0; j < kHeadsMax / 2; ++j)
                        if (j * 2 < H) {
                            const float2 w = *reinterpret_cast<const float2*>(src + j * 2);
                            pv[j * 2] = w.x, pv[j * 2 + 1] = w.y;
                        }
                } else {
#pragma unroll
                    for (int i = 0; i < kHeadsMax; ++i)
                        if (i < H) pv[i] = src[i];
                }
            }
            if (p + kTile < we) po = load_csr(a.order + p + kTile);
            return;
        }
        // the tile's weights: words [base H, min(base + 64, we) H) of val, 64 consecutive words per load (nnz H < 2^31: no wrap)
        const uint32_t vb = (uint32_t)base * (uint32_t)H;
        const uint32_t vfull = vb + (uint32_t)(kTile * H), vlast = (uint32_t)we * (uint32_t)H;
        const uint32_t ve = vfull < vlast ? vfull : vlast;
#pragma unroll
        for (int i = 0; i < kHeadsMax; ++i) {
            const uint32_t q = vb + (uint32_t)(i * kTile + lane);
            if (q < ve) pv[i] = load_csr(a.val + q);
        }
    };
    auto publish_tile = [&]() {
        s_off[wave][lane] = (uint32_t)pc * rowbytes;
        if constexpr (ORDERED) {  // pv[] holds the H weights of entry `lane`: slots lane H .. lane H + H - 1
            float* dst = &s_val[wave][lane * H];
            if (H == 4 || H == 8) {  // (16-byte slots: one or two ds_write_b128, consecutive lanes on consecutive slots)
#pragma unroll
                for (int j = 0; j < kHeadsMax / 4; ++j)
                    if (j * 4 < H) *reinterpret_cast<float4*>(dst + j * 4) = make_float4(pv[j * 4], pv[j * 4 + 1], pv[j * 4 + 2], pv[j * 4 + 3]);
            } else {
#pragma unroll
                for (int i = 0; i < kHeadsMax; ++i)
                    if (i < H) dst[i] = pv[i];
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < kHeadsMax; ++i)
            if (i < H) s_val[wave][i * kTile + lane] = pv[i];
    };
    if constexpr (PLANNED) {
        const int task_id = rb * kWaves + wave;
        if (task_id >= a.ntasks) return;
        const int4 t = reinterpret_cast<const int4*>(a.tasks)[task_id];
        row_first = __builtin_amdgcn_readfirstlane(t.x);
        nrows = __builtin_amdgcn_readfirstlane(t.y);
        wb = __builtin_amdgcn_readfirstlane(t.z);
        we = __builtin_amdgcn_readfirstlane(t.w);
        rp_plan = a.rowptr[row_first + (lane <= nrows ? lane : nrows)];
        pm_plan = a.perm[row_first + (lane < nrows ? lane : nrows - 1)];
    } else {
        const int rpw = a.rpw;
        row_first = (rb * kWaves + wave) * rpw;
        if (row_first >= a.M) return;  // whole wavefront leaves together
        nrows = (a.M - row_first < rpw) ? a.M - row_first : rpw;
        // Row pointers of this wavefront's rows -> LDS (one coalesced load, rpw <= 32).
        const int rp = a.rowptr[row_first + (lane <= nrows ? lane : nrows)];
        if (lane <= kMaxRowsPerWave) s_ptr[wave][lane] = rp;
        wb = __builtin_amdgcn_readfirstlane(rp);
        we = __builtin_amdgcn_readlane(rp, nrows);
    }
    if constexpr (ORDERED) {
        if (wb + lane < we) po = load_csr(a.order + wb + lane);
    }
    fetch_tile_regs(wb);

    int t0 = wb;
    if constexpr (PLANNED) {  // (after the tile loads are on their way: the three loads of a planned task overlap)
        if (lane <= kMaxRowsPerWave) s_ptr[wave][lane] = rp_plan;
        if (lane < kMaxRowsPerWave) s_perm[wave][lane] = pm_plan;
    }
    publish_tile();
    fetch_tile_regs(t0 + kTile);
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

        float acc[S][E * V];
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int i = 0; i < E * V; ++i) acc[s][i] = 0.0f;

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
                    for (int s = 0; s < S; ++s) {
                        if constexpr (DT != 0) {
                            accumulate_x16<DT, true, V>(acc[s], v[j][s], bv[j][s]);
                        } else {
#pragma unroll
                            for (int i = 0; i < V; ++i) acc[s][i] = __builtin_fmaf(v[j][s], bv[j][s][i], acc[s][i]);
                        }
                    }
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
                        for (int s = 0; s < S; ++s) {
                            if constexpr (DT != 0) {
                                accumulate_x16<DT, true, V>(acc[s], v[j][s], bv[j][s]);
                            } else {
#pragma unroll
                                for (int i = 0; i < V; ++i) acc[s][i] = __builtin_fmaf(v[j][s], bv[j][s][i], acc[s][i]);
                            }
                        }
                    }
                }
            }
            if (be <= tend) break;  // every row of this batch ends inside the resident tile
            wave_lds_sync();        // all reads of the old tile are issued before it is overwritten
            t0 = tend;
            publish_tile();
            fetch_tile_regs(t0 + kTile);
            wave_lds_sync();
        }

        if (rowok) {
            int crow = row_first + r;
            if constexpr (PLANNED) crow = s_perm[wave][r];
            float* Crow = a.C + (size_t)crow * (size_t)a.N + col0;
#pragma unroll
            for (int s = 0; s < S; ++s)
                if (colok[s]) {
                    if constexpr (DT != 0) {
                        float words[V];
                        pack_x16<DT, V>(words, acc[s]);  // the one rounding of each sum
                        if (nts) store_vec<V, true>(Crow + s * (W * V), words);
                        else store_vec<V, false>(Crow + s * (W * V), words);
                    } else {
                        if (nts) store_vec<V, true>(Crow + s * (W * V), acc[s]);
                        else store_vec<V, false>(Crow + s * (W * V), acc[s]);
                    }
                }
        }
    }
}

// The grid of one launch at lane geometry (V, S, W): rows per wavefront in whole lane-group batches, grown while the grid would not fit,
// column tiles of W V S words, one wavefront per task in plan mode. false: nothing to launch (*items == 0) or the grid cannot fit.
template <int V, int S, int W, bool PLANNED>
static bool heads_launch_shape(const HeadsArgs& a, int rpw, HeadsArgs* args, int64_t* items) {
    constexpr int G = 64 / W;
    *args = a;
    if (rpw < G) rpw = G;
    if (rpw > kMaxRowsPerWave) rpw = kMaxRowsPerWave;
    rpw = rpw / G * G;
    args->ntile = (a.N + W * V * S - 1) / (W * V * S);
    while (rpw < kMaxRowsPerWave && (((int64_t)a.M + kWaves * rpw - 1) / (kWaves * rpw)) * args->ntile > kMaxGridBlocks) {
        rpw *= 2;  // (the grid must fit 2^32 threads: tasks grow, never past the kernel's row-pointer staging)
        if (rpw > kMaxRowsPerWave) rpw = kMaxRowsPerWave;
        rpw = rpw / G * G;
    }
    args->rpw = rpw;
    args->nblk = (int)(((int64_t)a.M + kWaves * rpw - 1) / (kWaves * rpw));
    if constexpr (PLANNED) args->nblk = (a.ntasks + kWaves - 1) / kWaves;  // plan mode: one wavefront per task
    *items = (int64_t)args->nblk * args->ntile;
    return *items > 0 && *items <= kMaxGridBlocks;
}

}  // namespace gespmm
