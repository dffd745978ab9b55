// spmm_max_arg.hip — the max reducer with argmax and its gradient (spmm_max_arg.h): the batch-stream kernel of spmm_stream.h with a
// position register next to every accumulator word (forward), and the same walk over CSC columns that compares the saved positions
// and adds grad_out where they match (backward). A translation unit of its own: the kernels of spmm_stream.h stay exactly what they are.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spmm_device.h"
#include "spmm_max_arg.h"

namespace gespmm {

// ----------------------------------------------------------------------------- the walk
//
// The structure is spmm_heads_kernel's (see there): a wavefront owns `rpw` consecutive segments (rows forward, CSC columns backward) =
// one contiguous range of the index array, segment pointers in LDS by one coalesced load, the range streams through a 64-entry LDS tile
// with the next tile prefetched in registers, segments are walked G = 64 / W at a time, U gathers back to back and one predicated tail
// group. What differs:
//   forward   the tile stages the byte offset of the entry's B row; the entry's POSITION is t0 + its tile slot, a wave-uniform value.
//             Every accumulator word has a position register: `if (b > acc) { acc = b; pos = p; }` is one compare and two selects.
//   backward  the tile stages the byte offset of the entry's row in arg / grad_out and order[q]. A lane gathers its arg vector for
//             every entry (U back to back) and loads grad_out only where one of its words equals order[q]: M N of the nnz N compares
//             match, so most of those gathers never issue — and those of one group of U entries issue together.
// A segment is walked by its W lanes from its first entry to its last: every output word is ONE sequential chain, in any geometry.
// LDS per workgroup: s_off 1 KB + s_ord 1 KB (backward) + s_ptr 528 B.

template <int V, int S, int W, int U, bool BACKWARD>
__global__ __launch_bounds__(kThreads) void max_arg_kernel(MaxArgArgs a) {
    constexpr int G = 64 / W;

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
        cbytes[s] = colok[s] ? (uint32_t)(col0 + s * W * V) * 4u : 0u;
    }
    const char* src = reinterpret_cast<const char*>(a.src);
    const char* argin = reinterpret_cast<const char*>(a.arg_in);
    const uint32_t rowbytes = (uint32_t)a.N * 4u;

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

        // Forward: one entry, its gathered vector in hand (tile slot kj, position t0 + kj).
        auto consume = [&](int kj, const float (&bv)[S][V]) {
            const int p = t0 + kj;
#pragma unroll
            for (int s = 0; s < S; ++s)
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const bool win = bv[s][i] > acc[s][i];  // false for NaN and for equal values: the first one stays
                    acc[s][i] = win ? bv[s][i] : acc[s][i];
                    pos[s][i] = win ? p : pos[s][i];
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
            float go[n][S][V];
#pragma unroll
            for (int j = 0; j < n; ++j) {
                if (hit[j] != 0u) {
                    const uint32_t off = s_off[wave][k + j];
#pragma unroll
                    for (int s = 0; s < S; ++s) load_vec<V>(go[j][s], src + (uint32_t)(off + cbytes[s]));
                }
            }
#pragma unroll
            for (int j = 0; j < n; ++j) {
                if (hit[j] != 0u) {
#pragma unroll
                    for (int s = 0; s < S; ++s)
#pragma unroll
                        for (int i = 0; i < V; ++i) acc[s][i] = ((hit[j] >> (s * V + i)) & 1u) ? acc[s][i] + go[j][s][i] : acc[s][i];
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
                float bv[U][S][V];
#pragma unroll
                for (int j = 0; j < U; ++j) off[j] = s_off[wave][k + j];
#pragma unroll
                for (int j = 0; j < U; ++j)
#pragma unroll
                    for (int s = 0; s < S; ++s) load_vec<V>(bv[j][s], gather + (uint32_t)(off[j] + cbytes[s]));
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
                float bv[U - 1][S][V];
#pragma unroll
                for (int j = 0; j < U - 1; ++j) off[j] = s_off[wave][k + ((j < rem) ? j : rem - 1)];
#pragma unroll
                for (int j = 0; j < U - 1; ++j) {
                    if (j < rem) {
#pragma unroll
                        for (int s = 0; s < S; ++s) load_vec<V>(bv[j][s], gather + (uint32_t)(off[j] + cbytes[s]));
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
                    store_vec<V, false>(a.dst + word0 + s * (W * V), acc[s]);
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

// ----------------------------------------------------------------------------- launch table

template <int V, int S, int W, bool BACKWARD>
static hipError_t launch_max_arg(const MaxArgArgs& a, int rpw, hipStream_t st) {
    constexpr int G = 64 / W;
    // gather depth, as launch_heads (spmm_heads.hip). The backward keeps one compare mask per word of a group in scalar registers until
    // the group's adds: four entries per group from four words per lane on, or the masks no longer fit
    constexpr int U = (V * S >= (BACKWARD ? 4 : 8)) ? 4 : 8;
    MaxArgArgs args = a;
    if (rpw < G) rpw = G;
    if (rpw > kMaxRowsPerWave) rpw = kMaxRowsPerWave;
    rpw = rpw / G * G;
    args.ntile = (a.N + W * V * S - 1) / (W * V * S);
    while (rpw < kMaxRowsPerWave && (((int64_t)a.S + kWaves * rpw - 1) / (kWaves * rpw)) * args.ntile > kMaxGridBlocks) {
        rpw *= 2;  // (the grid must fit 2^32 threads: tasks grow, never past the kernel's pointer staging)
        if (rpw > kMaxRowsPerWave) rpw = kMaxRowsPerWave;
        rpw = rpw / G * G;
    }
    args.rpw = rpw;
    args.nblk = (int)(((int64_t)a.S + kWaves * rpw - 1) / (kWaves * rpw));
    const int64_t nitems = (int64_t)args.nblk * args.ntile;
    if (nitems <= 0) return hipSuccess;
    if (nitems > kMaxGridBlocks) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL((max_arg_kernel<V, S, W, U, BACKWARD>), dim3((unsigned)nitems), dim3(kThreads), 0, st, args);
    return hipGetLastError();
}

template <bool BACKWARD>
static hipError_t launch_max_arg_geometry(const MaxArgArgs& a, const Geometry& g, hipStream_t st) {
    if (!max_arg_geometry_served(g)) return hipErrorInvalidValue;
#define GESPMM_MAX_ARG(V_, S_, W_) \
    if (g.vec == V_ && g.strips == S_ && g.group == W_) return launch_max_arg<V_, S_, W_, BACKWARD>(a, g.rows_per_wave, st);
    GESPMM_MAX_ARG(1, 1, 4)
    GESPMM_MAX_ARG(1, 1, 8)
    GESPMM_MAX_ARG(1, 1, 16)
    GESPMM_MAX_ARG(1, 1, 32)
    GESPMM_MAX_ARG(1, 1, 64)
    GESPMM_MAX_ARG(4, 1, 32)
    GESPMM_MAX_ARG(4, 1, 64)
    GESPMM_MAX_ARG(4, 2, 64)
    GESPMM_MAX_ARG(2, 1, 64)
    GESPMM_MAX_ARG(2, 2, 64)
    GESPMM_MAX_ARG(1, 2, 64)
#undef GESPMM_MAX_ARG
    return hipErrorInvalidValue;
}

hipError_t launch_spmm_max_arg(const MaxArgArgs& a, const Geometry& geo, hipStream_t st) {
    return launch_max_arg_geometry<false>(a, geo, st);
}

hipError_t launch_spmm_max_backward(const MaxArgArgs& a, const Geometry& geo, hipStream_t st) {
    return launch_max_arg_geometry<true>(a, geo, st);
}

}  // namespace gespmm
