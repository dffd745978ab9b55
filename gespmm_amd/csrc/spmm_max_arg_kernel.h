// spmm_max_arg_kernel.h — the body of the max reducer's two kernels (spmm_max_arg.h) as a template on the ELEMENT TYPE of the dense
// operands, and the grid of its launch. DT = kX16F16 / kX16Bf16: gespmm_csr_spmm_max_arg_x16 / gespmm_csr_spmm_max_backward_x16
// (spmm_max_arg_x16.hip). DT = 0 is the fp32 body, expression for expression what stands in spmm_max_arg.hip.
//
// The walk is spmm_max_arg.hip's (see there): `rpw` segments per wavefront, a 64-entry LDS tile one tile ahead, W lanes per segment, U
// gathers back to back and one predicated tail group; every output word is ONE sequential chain, in any geometry.
//
// 16-bit elements (DT != 0). The geometry counts ELEMENTS: a lane holds V of them per strip, so the columns a lane owns, the positions,
// the arg words and their 4 V-byte loads and stores are the fp32 kernel's. What differs is the width of the other operand:
//   forward   the tile stages colind[p] N 2, the byte offset of the entry's B row; a gather is ONE load of 2 V bytes (2 / 4 / 8) and
//             the vector stays packed until its compare: widen (exact), `b > acc` in fp32 against the fp32 accumulator — which starts
//             at empty_value as given, whether the type can hold it or not — and the row-end store narrows each word once (to nearest
//             even) and writes 2 V bytes. V = 1 stores are 2-byte stores: neighbouring lanes write the two halves of a dword.
//   backward  the tile stages ONE offset per entry, r N 4 of the arg row; grad_out's row starts at half of it: (off + 4 c) >> 1. The
//             gathers under the hit mask are 2 V-byte loads kept packed until the adds; g is an fp32 chain narrowed once at the store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "spmm_device.h"
#include "spmm_max_arg.h"

namespace gespmm {

// V 16-bit elements in (V + 1) / 2 registers: the lower-addressed element in the low half of its word (V = 1: the low half alone).
template <int V>
__device__ __forceinline__ void load_x16_vec(uint32_t (&w)[(V + 1) / 2], const char* p) {
    if constexpr (V == 1) {
        w[0] = *reinterpret_cast<const uint16_t*>(p);
    } else if constexpr (V == 2) {
        w[0] = *reinterpret_cast<const uint32_t*>(p);
    } else {
        static_assert(V == 4, "V = 8 (16-byte loads) is not built");
        using T = uint32_t __attribute__((ext_vector_type(2)));
        const T v = *reinterpret_cast<const T*>(p);
        w[0] = v[0];
        w[1] = v[1];
    }
}

template <int DT, int V>
__device__ __forceinline__ void widen_x16_vec(float (&f)[V], const uint32_t (&w)[(V + 1) / 2]) {
    if constexpr (V == 1) {
        float hi;
        widen_x16<DT>(__uint_as_float(w[0]), f[0], hi);
    } else {
#pragma unroll
        for (int i = 0; i < V / 2; ++i) widen_x16<DT>(__uint_as_float(w[i]), f[2 * i], f[2 * i + 1]);
    }
}

// The one rounding of each word, and one store of 2 V bytes.
template <int DT, int V>
__device__ __forceinline__ void store_x16_vec(char* p, const float (&acc)[V]) {
    if constexpr (V == 1) {
        *reinterpret_cast<uint16_t*>(p) = (uint16_t)narrow_x16<DT>(acc[0]);
    } else if constexpr (V == 2) {
        *reinterpret_cast<uint32_t*>(p) = narrow_x16<DT>(acc[0]) | (narrow_x16<DT>(acc[1]) << 16);
    } else {
        using T = uint32_t __attribute__((ext_vector_type(2)));
        T v;
        v[0] = narrow_x16<DT>(acc[0]) | (narrow_x16<DT>(acc[1]) << 16);
        v[1] = narrow_x16<DT>(acc[2]) | (narrow_x16<DT>(acc[3]) << 16);
        *reinterpret_cast<T*>(p) = v;
    }
}

template <int DT, int V, int S, int W, int U, bool BACKWARD>
__global__ __launch_bounds__(kThreads) void max_arg_kernel_t(MaxArgArgs a) {
    constexpr int G = 64 / W;
    constexpr bool X16 = DT != 0;
    constexpr bool PACKED = X16 && !BACKWARD;  // the main loop gathers 16-bit vectors (forward); arg words otherwise (backward)
    constexpr int GV = PACKED ? (V + 1) / 2 : V;
    constexpr int PV = X16 ? (V + 1) / 2 : V;  // registers of one gathered vector of the 16-bit (or fp32) operand
    constexpr uint32_t kGatherElem = PACKED ? 2u : 4u;
    using gather_t = std::conditional_t<PACKED, uint32_t, float>;
    using packed_t = std::conditional_t<X16, uint32_t, float>;

    __shared__ uint32_t s_off[kWaves][kTile];
    __shared__ int s_ord[BACKWARD ? kWaves : 1][BACKWARD ? kTile : 1];
    __shared__ int s_ptr[kWaves][kMaxRowsPerWave + 1];

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / W;
    const int l = lane % W;

    const int nitems = a.nblk * a.ntile;
    const int item = xcd_contiguous(blockIdx.x, nitems);
    int tile = 0, rb = item;
    if (a.ntile > 1) {
        tile = item % a.ntile;
        rb = item / a.ntile;
    }

    const int col0 = tile * (W * V * S) + l * V;
    bool colok[S];
    uint32_t cbytes[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        colok[s] = (col0 + s * W * V) < a.N;
        // lanes/strips past N gather column 0 (valid, same line as lane 0) and skip the store
        cbytes[s] = colok[s] ? (uint32_t)(col0 + s * W * V) * kGatherElem : 0u;
    }
    const char* src = reinterpret_cast<const char*>(a.src);
    const char* argin = reinterpret_cast<const char*>(a.arg_in);
    const uint32_t rowbytes = (uint32_t)a.N * kGatherElem;

    const int rpw = a.rpw;
    const int seg_first = (rb * kWaves + wave) * rpw;
    if (seg_first >= a.S) return;  // whole wavefront leaves together
    const int nseg = (a.S - seg_first < rpw) ? a.S - seg_first : rpw;
    // Pointers of this wavefront's segments -> LDS (one coalesced load, rpw <= 32).
    const int rp = a.ptr[seg_first + (lane <= nseg ? lane : nseg)];
    if (lane <= kMaxRowsPerWave) s_ptr[wave][lane] = rp;
    const int wb = __builtin_amdgcn_readfirstlane(rp);
    const int we = __builtin_amdgcn_readlane(rp, nseg);

    // Tile stream state: `t0` = position of the tile resident in LDS.
    int pc = 0, po = 0;
    auto fetch_tile_regs = [&](int base) {
        const int p = base + lane;
        if (p < we) {
            pc = load_csr(a.ind + p);
            if constexpr (BACKWARD) po = load_csr(a.order + p);
        }
    };
    auto publish_tile = [&]() {
        s_off[wave][lane] = (uint32_t)pc * rowbytes;
        if constexpr (BACKWARD) s_ord[wave][lane] = po;
    };

    fetch_tile_regs(wb);
    int t0 = wb;
    publish_tile();
    fetch_tile_regs(t0 + kTile);
    wave_lds_sync();

    for (int b = 0; b < nseg; b += G) {
        const int r = b + g;
        const bool segok = r < nseg;
        int lb = 0, hb = 0;
        if (segok) {
            lb = s_ptr[wave][r];
            hb = s_ptr[wave][r + 1];
        }
        const int be = __builtin_amdgcn_readfirstlane(s_ptr[wave][(b + G < nseg) ? b + G : nseg]);
        if constexpr (G == 1) {
            lb = __builtin_amdgcn_readfirstlane(lb);
            hb = __builtin_amdgcn_readfirstlane(hb);
        }

        float acc[S][V];
        int pos[S][V];
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int i = 0; i < V; ++i) {
                acc[s][i] = BACKWARD ? 0.0f : a.empty;
                pos[s][i] = -1;
            }

        auto gather_vec = [&](gather_t(&dst)[GV], const char* p) {
            if constexpr (PACKED) load_x16_vec<V>(dst, p);
            else load_vec<V>(dst, p);
        };
        // Forward: one entry, its gathered vector in hand (tile slot kj, position t0 + kj).
        auto consume = [&](int kj, const gather_t (&bv)[S][GV]) {
            const int p = t0 + kj;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                float f[V];
                if constexpr (PACKED) {
                    widen_x16_vec<DT, V>(f, bv[s]);
                } else {
#pragma unroll
                    for (int i = 0; i < V; ++i) f[i] = bv[s][i];
                }
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const bool win = f[i] > acc[s][i];  // false for NaN and for equal values: the first one stays
                    acc[s][i] = win ? f[i] : acc[s][i];
                    pos[s][i] = win ? p : pos[s][i];
                }
            }
        };
        // Backward: a group of `cnt` entries (tile slots k ..), their arg vectors in hand. Three passes, so that the grad_out gathers of
        // the group are in flight together instead of one round trip per entry: the compares (one bit per word), the gathers of the
        // entries with a hit — rare: under the exec mask of the lanes that matched — and the adds, in entry order.
        auto scatter_group = [&](int k, int cnt, auto& bv) {
            constexpr int n = sizeof(bv) / sizeof(bv[0]);
            uint32_t hit[n];
#pragma unroll
            for (int j = 0; j < n; ++j) {
                hit[j] = 0u;
                if (j < cnt) {
                    const int want = s_ord[wave][k + j];
#pragma unroll
                    for (int s = 0; s < S; ++s)
#pragma unroll
                        for (int i = 0; i < V; ++i) hit[j] |= (uint32_t)(__float_as_int(bv[j][s][i]) == want) << (s * V + i);
                }
            }
            packed_t go[n][S][PV];
#pragma unroll
            for (int j = 0; j < n; ++j) {
                if (hit[j] != 0u) {
                    const uint32_t off = s_off[wave][k + j];
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        // (16-bit: the staged offset and cbytes are arg's, r N 4 and 4 c; grad_out's are half of them)
                        if constexpr (X16) load_x16_vec<V>(go[j][s], src + (uint32_t)((off + cbytes[s]) >> 1));
                        else load_vec<V>(go[j][s], src + (uint32_t)(off + cbytes[s]));
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < n; ++j) {
                if (hit[j] != 0u) {
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        float f[V];
                        if constexpr (X16) {
                            widen_x16_vec<DT, V>(f, go[j][s]);
                        } else {
#pragma unroll
                            for (int i = 0; i < V; ++i) f[i] = go[j][s][i];
                        }
#pragma unroll
                        for (int i = 0; i < V; ++i) acc[s][i] = ((hit[j] >> (s * V + i)) & 1u) ? acc[s][i] + f[i] : acc[s][i];
                    }
                }
            }
        };
        const char* gather = BACKWARD ? argin : src;  // (arg words travel in float registers: loads and moves keep every bit)

        for (;;) {
            const int tend = t0 + kTile;
            int k = (lb > t0 ? lb : t0) - t0;
            const int ke = (hb < tend ? hb : tend) - t0;
            // Full steps: U gathers issued back to back, no predicates.
            for (; k + U <= ke; k += U) {
                uint32_t off[U];
                gather_t bv[U][S][GV];
#pragma unroll
                for (int j = 0; j < U; ++j) off[j] = s_off[wave][k + j];
#pragma unroll
                for (int j = 0; j < U; ++j)
#pragma unroll
                    for (int s = 0; s < S; ++s) gather_vec(bv[j][s], gather + (uint32_t)(off[j] + cbytes[s]));
                if constexpr (BACKWARD) {
                    scatter_group(k, U, bv);
                } else {
#pragma unroll
                    for (int j = 0; j < U; ++j) consume(k + j, bv[j]);
                }
            }
            // Tail (1..U-1 entries): ONE predicated group; LDS reads first (clamped slot: always inside the tile), then the gathers.
            const int rem = ke - k;
            if (rem > 0) {
                uint32_t off[U - 1];
                gather_t bv[U - 1][S][GV];
#pragma unroll
                for (int j = 0; j < U - 1; ++j) off[j] = s_off[wave][k + ((j < rem) ? j : rem - 1)];
#pragma unroll
                for (int j = 0; j < U - 1; ++j) {
                    if (j < rem) {
#pragma unroll
                        for (int s = 0; s < S; ++s) gather_vec(bv[j][s], gather + (uint32_t)(off[j] + cbytes[s]));
                    }
                }
                if constexpr (BACKWARD) {
                    scatter_group(k, rem, bv);
                } else {
#pragma unroll
                    for (int j = 0; j < U - 1; ++j) {
                        if (j < rem) consume(k + j, bv[j]);
                    }
                }
            }
            if (be <= tend) break;  // every segment of this batch ends inside the resident tile
            wave_lds_sync();        // all reads of the old tile are issued before it is overwritten
            t0 = tend;
            publish_tile();
            fetch_tile_regs(t0 + kTile);
            wave_lds_sync();
        }

        if (segok) {
            const size_t word0 = (size_t)(seg_first + r) * (size_t)a.N + (size_t)col0;
#pragma unroll
            for (int s = 0; s < S; ++s)
                if (colok[s]) {
                    if constexpr (X16) store_x16_vec<DT, V>(reinterpret_cast<char*>(a.dst) + (word0 + s * (W * V)) * 2, acc[s]);
                    else store_vec<V, false>(a.dst + word0 + s * (W * V), acc[s]);
                    if constexpr (!BACKWARD) {
                        float pw[V];
#pragma unroll
                        for (int i = 0; i < V; ++i) pw[i] = __int_as_float(pos[s][i]);
                        store_vec<V, false>(reinterpret_cast<float*>(a.arg_out) + word0 + s * (W * V), pw);
                    }
                }
        }
    }
}

// The grid of one launch at lane geometry (V, S, W): segments per wavefront in whole lane-group batches, grown while the grid would not
// fit, column tiles of W V S elements. false: nothing to launch (*items <= 0) or the grid cannot fit.
template <int V, int S, int W>
static bool max_arg_launch_shape(const MaxArgArgs& a, int rpw, MaxArgArgs* args, int64_t* items) {
    constexpr int G = 64 / W;
    *args = a;
    if (rpw < G) rpw = G;
    if (rpw > kMaxRowsPerWave) rpw = kMaxRowsPerWave;
    rpw = rpw / G * G;
    args->ntile = (a.N + W * V * S - 1) / (W * V * S);
    while (rpw < kMaxRowsPerWave && (((int64_t)a.S + kWaves * rpw - 1) / (kWaves * rpw)) * args->ntile > kMaxGridBlocks) {
        rpw *= 2;  // (the grid must fit 2^32 threads: tasks grow, never past the kernel's pointer staging)
        if (rpw > kMaxRowsPerWave) rpw = kMaxRowsPerWave;
        rpw = rpw / G * G;
    }
    args->rpw = rpw;
    args->nblk = (int)(((int64_t)a.S + kWaves * rpw - 1) / (kWaves * rpw));
    *items = (int64_t)args->nblk * args->ntile;
    return *items > 0 && *items <= kMaxGridBlocks;
}

}  // namespace gespmm
