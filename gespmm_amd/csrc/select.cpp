// select.cpp — variant and geometry selection.
//
// The reference dispatches on N alone (spmm_kernel.cu:186-206, 437-457):
//   N < 32 -> naive, 32 <= N < 64 -> CRC, N >= 64 -> CRC + CWM(2).
// On a 64-lane wavefront that table wastes lanes for every N < 64, so the
// geometry here is derived instead: the widest contiguous vector the row stride
// allows (V), then just enough lanes per row (W) to cover N, and the remaining
// 64/W lane groups take further rows.

#include "select.h"

#include "../../include/gespmm.h"

namespace gespmm {

static int pow2_ceil(int64_t x) {
    int p = 1;
    while (p < x && p < 64) p <<= 1;
    return p;
}

int auto_variant(int64_t M, int64_t nnz, int64_t N) {
    (void)nnz;
    // Up to 64 columns one lane per column already spans a whole wavefront-wide group;
    // coarsening would only shrink the group and put more rows on one wavefront, and a
    // 64-entry CSR tile of a long row feeds ONE group at a time. Measured (profiles/r01/
    // narrow_n_kernel_choice.log): V=1 is equal or faster for every graph at N <= 64,
    // by 30-58 % on the denser ones (products-like N=32, reddit-like N<=32).
    if (N <= 64) return GESPMM_VARIANT_CRC;
    // Just above one 256-column tile the second tile would be mostly empty yet walk every row again:
    // two strips per lane (one 512-column tile) instead — 24 % faster at N = 260, 3 % at 384 on a
    // 335 k-row graph; small graphs prefer the extra workgroups of two tiles (profiles/r01/width_audit.log).
    if (N % 4 == 0 && N > 256 && N <= 384 && M >= (1 << 17)) return GESPMM_VARIANT_CRC_CWM8;
    if (N % 4 == 0) return GESPMM_VARIANT_CRC_CWM4;
    if (N % 2 == 0) return GESPMM_VARIANT_CRC_CWM2;
    return GESPMM_VARIANT_CRC;
}

int resolve_geometry(int64_t M, int64_t K, int64_t N, int64_t nnz, int variant, int max_vec,
                     int cfg_vec, int cfg_strips, int cfg_group, int cfg_rows_per_wave, int cfg_slab_rows, int flags,
                     Selection* out) {
    if (variant == GESPMM_VARIANT_AUTO) {
        variant = auto_variant(M, nnz, N);
        // Opt-in (GESPMM_FLAG_ALLOW_REASSOCIATION): narrow N on dense rows is 1.3-2x faster with
        // lanes spread over the non-zeros (variant 5) — a re-ordered sum, within 1e-4, not bit-exact.
        if ((flags & kFlagAllowReassoc) && N <= 16 && nnz > 0 && M > 0 && nnz / M >= 32)
            variant = GESPMM_VARIANT_PARREDUCE;
    }
    Geometry g;
    g.reduce = kReduceSum;
    g.idx64 = ((flags & kFlagForceIdx64) != 0) || ((uint64_t)K * (uint64_t)N * 4ull >= (1ull << 32));
    g.strips = 1;
    switch (variant) {
        case GESPMM_VARIANT_NAIVE:
        case GESPMM_VARIANT_CRC: g.vec = 1; break;
        case GESPMM_VARIANT_CRC_CWM2: g.vec = 2; break;
        case GESPMM_VARIANT_CRC_CWM4: g.vec = 4; break;
        case GESPMM_VARIANT_CRC_CWM8: g.vec = 4; g.strips = 2; break;
        case GESPMM_VARIANT_PARREDUCE: g.vec = 1; break;
        default: return GESPMM_EINVAL;
    }
    if (cfg_vec) {
        if (cfg_vec != 1 && cfg_vec != 2 && cfg_vec != 4) return GESPMM_EINVAL;
        g.vec = cfg_vec;
    }
    if (cfg_strips) {
        if (cfg_strips != 1 && cfg_strips != 2) return GESPMM_EINVAL;
        g.strips = cfg_strips;
    }
    // Degrade to what alignment and N allow; results do not depend on V/S/W.
    if (g.vec > max_vec) g.vec = max_vec;
    if (g.strips == 2 && g.vec != 4) g.strips = 1;
    // Widths with no dwordx4 access (odd N, N = 2 mod 4, or unaligned operands) beyond one 64-lane tile: two
    // strips per lane halve the number of column tiles — each tile walks every entry of every row again
    // (reddit-like N = 65: 5.3 -> 3.9 ms; bench graph N = 513: 719 -> 647 us; no gain where scalar gathers are issue-bound, N = 127; profiles/r01/width_audit.log). Batch-stream, blocked and
    // long-row kernels only; W = 64.
    const bool wide_narrow_vec = g.vec < 4 && cfg_strips == 0 && cfg_group == 0 && N > 64 * g.vec &&
                                 variant != GESPMM_VARIANT_NAIVE && variant != GESPMM_VARIANT_PARREDUCE &&
                                 (flags & kFlagSegStream) == 0;
    if (wide_narrow_vec) g.strips = 2;

    if (variant == GESPMM_VARIANT_PARREDUCE) {
        const int64_t avg = (nnz > 0 && M > 0) ? (nnz + M - 1) / M : 16;
        g.group = pow2_ceil(avg);
    } else {
        const int64_t per_lane = (int64_t)g.vec * g.strips;
        g.group = pow2_ceil((N + per_lane - 1) / per_lane);
    }
    if (g.group < 4) g.group = 4;
    if (cfg_group) {
        if (cfg_group < 4 || cfg_group > 64 || (cfg_group & (cfg_group - 1))) return GESPMM_EINVAL;
        g.group = cfg_group;
    }
    // Rows per wavefront of the batch-stream kernel. Measured over the graph families at
    // N = 32..512 (profiles/r01/rows_per_wave_sweep.log): the best task size is ~12 KB of B
    // gathered per wavefront task — 96 CSR entries at N = 32, 24 at N = 128 — never fewer
    // than 16 entries; larger tasks lose 5-17 % (coarser dynamic balance over the CUs).
    // (grid depth: see below)
    const int rows_in_flight = 64 / g.group;
    const bool b_resident = (uint64_t)K * (uint64_t)N * 4ull <= (8ull << 20);
    {
        const int64_t avg = (nnz > 0 && M > 0) ? (nnz + M - 1) / M : 8;
        const int64_t tile_cols = (int64_t)g.group * g.vec * g.strips;
        const int64_t entry_bytes = 4 * (N < tile_cols ? N : tile_cols);
        int64_t target = (12 << 10) / (entry_bytes > 0 ? entry_bytes : 4);
        if (target < 16) target = 16;
        if (target > 96) target = 96;
        // B small enough to live in the L2s: the kernel is issue-bound, not fabric-bound, and the
        // per-task prologue counts — larger tasks (73-82 vs 97 us at K = 2048, cache_regime_sweep*.log)
        if (b_resident) target = 128;
        int rpw = kMaxRowsPerWave;
        while (rpw > rows_in_flight && (int64_t)rpw * avg > target) rpw >>= 1;
        // ... but never fewer wavefronts than the chip has slots (256 CUs x 32): one full round
        while (rpw > rows_in_flight && M / rpw < 8192) rpw >>= 1;
        if (rpw < rows_in_flight) rpw = rows_in_flight;
        g.rows_per_wave = rpw;
    }
    // Rows per lane group of the segmented-stream kernel: ~64 CSR entries per group task
    // (two 32-entry tiles), again keeping the grid several waves deep.
    {
        const int64_t avg = (nnz > 0 && M > 0) ? (nnz + M - 1) / M : 8;
        int rpg = kMaxRowsPerWave;
        while (rpg > 1 && (int64_t)rpg * avg > 64) rpg >>= 1;
        while (rpg > 1 && M / ((int64_t)rpg * rows_in_flight) < 4 * 8192) rpg >>= 1;
        if (b_resident && rpg > 4) rpg = 4;  // kernel_generations_cache_regimes.log: g4 58 us, g8 65
        g.rows_per_group = rpg;
    }
    if (cfg_rows_per_wave) {
        g.rows_per_wave = cfg_rows_per_wave;
        g.rows_per_group = cfg_rows_per_wave;
    }
    // Kernel generation. Wide groups (W >= 32: one or two rows per wavefront) run the
    // segmented-stream kernel; with many narrow groups per wavefront its per-entry row
    // flushes diverge between groups and the batch kernel (rows in lock-step, one store
    // phase per batch) is faster — measured in profiles/r01/kernel_generations.log.
    const int64_t avg_deg = (nnz > 0 && M > 0) ? (nnz + M - 1) / M : 8;
    // Cache blocking for dense graphs (one launch per ~6 MB column slab of B, see
    // spmm_kernels.hip): worth it when B per column tile is much larger than an L2 and a
    // row still carries enough work in every slab.
    {
        auto plan = [&](int64_t row_bytes, int64_t* slab_rows_out, int64_t* nslab_out) {
            int64_t slab_rows = cfg_slab_rows > 0 ? cfg_slab_rows : (6 << 20) / row_bytes;
            if (slab_rows < 64 && cfg_slab_rows <= 0) slab_rows = 64;
            if (slab_rows > 0x3fffffff) slab_rows = 0x3fffffff;
            const int64_t nslab = (K + slab_rows - 1) / slab_rows;
            *slab_rows_out = slab_rows;
            *nslab_out = nslab;
            // Measured (profiles/r01/slab_blocking.log, heuristic_audit.log, dense_width_audit.log): blocking wins
            // when the part of a row that falls into one slab still gathers >= ~10 KB (reddit-like: 13 KB at every
            // width; a 200 k-row degree-150 matrix: 4.5 KB, 27 % slower blocked) — with 6 MB slabs that is a matrix
            // density of ~0.16 %. Below it the per-slab read-modify-write of C outweighs the L2 hits. Also: B at
            // least 4 slabs, mean degree >= 64, row slices >= 256 B (a loss at N = 32).
            return nnz > 0 && M > 0 && row_bytes >= 256 && nslab >= 4 && nslab <= 4096 && avg_deg >= 64 &&
                   avg_deg * row_bytes >= 10240 * nslab;
        };
        int64_t slab_rows = 0, nslab = 0;
        bool dense;
        const bool forced = (flags & kFlagSlabBlocked) != 0;
        if (g.vec == 4 && N > 128 && cfg_strips == 0 && cfg_group == 0) {
            // The blocked path picks its own column tiling (a tile with few live columns costs as much as a full
            // one: every tile walks every entry). Column tiles are dealt to workgroups round-robin (tile = id mod
            // ntile) and workgroup ids to XCDs round-robin (id mod 8), so with 2, 4 or 8 FULL 128-column tiles
            // an XCD only ever sees one tile and its L2 holds slab_rows x 512 B: N = 256 / 512 / 1024 use
            // 512-byte tiles (N = 256: 9.96 -> 8.79 ms on reddit-like, slab_size_sweep_v2.log). Every other
            // width takes ceil(N / 256) tiles of 1 KB (N = 132: 8.9 -> 6.6 ms, N = 384: 23.8 -> 17.1,
            // N = 516: 43 -> 30, dense_width_audit.log).
            const int64_t ntile128 = (N + 127) / 128;
            const bool xcd_tiles = (N % 128 == 0) && (ntile128 == 2 || ntile128 == 4 || ntile128 == 8);
            dense = plan(xcd_tiles ? 512 : 1024, &slab_rows, &nslab);
            if (dense || forced) {
                g.group = xcd_tiles ? 32 : 64;
                g.strips = 1;
                if (variant == GESPMM_VARIANT_CRC_CWM8) variant = GESPMM_VARIANT_CRC_CWM4;  // report what runs
            }
        } else {
            dense = plan((int64_t)g.group * g.vec * g.strips * 4, &slab_rows, &nslab);
        }
        g.slab_rows = (int)slab_rows;
        g.K = K;
        g.slab_blocked = (forced || dense) && (flags & kFlagNoSlabBlocked) == 0 && nslab <= 65536 &&
                         variant != GESPMM_VARIANT_NAIVE && variant != GESPMM_VARIANT_PARREDUCE;
    }
    // (needs nnz to size its workspace: callers that pass nnz = -1 keep the strict chain)
    // The pass costs ~6.5 us of extra launches when there is no long row (profiles/r01/longrow_threshold_audit.log),
    // and the host cannot see the degrees. Always on from 2^23 entries; from 2^20 when the mean degree is >= 8
    // (RMAT-16..18: 1.8-5x faster with it; com-Amazon-shaped graphs, mean degree 5.5 and no hubs, keep their 150 us).
    // Smaller or sparser matrices with hub rows: GESPMM_FLAG_SPLIT_LONG_ROWS.
    const bool auto_split = nnz >= kLongRowMinNnz || (nnz >= (1 << 20) && M > 0 && nnz / M >= 8);
    g.split_long_rows = nnz > 0 && ((flags & kFlagSplitLongRows) != 0 || auto_split) && (flags & kFlagStrictOrder) == 0 &&
                        variant != GESPMM_VARIANT_NAIVE && variant != GESPMM_VARIANT_PARREDUCE;
    // A row is "long" when it dwarfs the average wavefront's work: 32x the mean degree,
    // at least kLongRowThreshold entries (reddit-like graphs, mean degree ~500, keep
    // their many 2k..15k-entry rows on the main kernel, which is faster on them).
    {
        int64_t thr = 32 * avg_deg;
        if (thr < kLongRowThreshold) thr = kLongRowThreshold;
        if (thr > 0x3fffffff) thr = 0x3fffffff;
        g.long_row_threshold = (int)thr;
    }
    // With task sizes tuned per kernel the batch kernel is equal or faster on every graph family
    // whose B exceeds the L2s (profiles/r01/rows_per_wave_sweep.log), and it implements the long-row
    // split. The segmented kernel keeps the short-row, L2-resident-B corner (58 vs 68 us,
    // kernel_generations_cache_regimes.log) and is otherwise opt-in (GESPMM_FLAG_SEG_STREAM).
    // ... and very short rows (mean degree <= 3: road-network-like), where the batch kernel spends a dependent round trip per
    // row pair and the continuous stream runs at copy speed (M = 335 k, N = 128, every row 1 / 2 / 3 entries: 64-69 / 76 / 98 us vs
    // 79-82 / 91 / 101 us; degrees 1..8 mixed, mean 2.75: 92 vs 102 us; profiles/r02/low_degree_floor.log)
    g.segmented = ((flags & kFlagSegStream) != 0 || (b_resident && g.group >= 32 && avg_deg <= 12) ||
                   (g.group >= 32 && avg_deg <= 3 && M >= (1 << 16))) &&
                  !g.split_long_rows && !(g.strips == 2 && g.vec < 4);
    // System-scope C stores (GESPMM_FLAG_SC1_STORE) stay opt-in: with B L2-resident and C not, they help when the reuse of B is
    // skewed (the BENCH graph's rows folded onto a 1 MB B: 81 -> 65 us; 4 MB: 86 -> 82) and cost when it is uniform and store-heavy
    // (uniform degree 6 over the same B: 54.5 -> 61.9 us; 73.7 -> 75.6) — profiles/r02/l2_resident_store_scope.log. The host
    // cannot tell the two apart without reading the matrix.
    g.sc1_store = false;
    out->variant = variant;
    out->geo = g;
    return 0;
}

// Row-walking (one wavefront per row) is skew-sensitive — a hub row is walked by one wavefront — and only pays
// for long rows: parity with the edge-parallel form at degree 32-48, up to 2x at degree >= 64 on patterns too
// small to block (profiles/r01/sddmm_heuristic_audit.log).
constexpr int64_t kSddmmRowWalkMinDegree = 64;

SddmmLaunch resolve_sddmm(bool csr, int64_t M, int64_t nnz, int64_t N, int d1_align, int d2_align, bool capturing, int elem_size) {
    const int64_t es = elem_size;  // 4: fp32; 2: fp16 / bf16 — V counts elements, the rules below are about bytes
    SddmmLaunch r = {csr ? kSddmmCsrEdge : kSddmmCooEdge, (int)(16 / es), 4, 0, 0, 0};
    while (r.V > 1 && ((N % r.V) != 0 || (d1_align % (es * r.V)) != 0 || (d2_align % (es * r.V)) != 0)) r.V >>= 1;
    // Lanes per edge: a lane walks ~2 dwordx4 vectors (~32 bytes, at most 8 loads: 8 scalars when the rows allow no vector loads)
    // of both rows, so a wavefront has 64/W edges in flight and the butterfly is log2(W) steps.
    // Measured against "just enough lanes to cover N" (profiles/r01/sddmm_group_width.log):
    // N=41 2.4-2.8x, N=64 1.35x, N=128 1.2x faster on reddit-like, equal or better on com-Amazon-like.
    // Every form uses the same width, so COO, CSR and the cache-blocked form agree bit for bit.
    // (fp32: 2 / 4 / 8 vectors for V = 4 / 2 / 1; 16 bits: 2 / 4 / 8 / 8 for V = 8 / 4 / 2 / 1 — carried over, not measured at 16 bits)
    const int64_t per_lane = (32 / (es * r.V) < 8) ? 32 / (es * r.V) : 8;
    while (r.W < 64 && (int64_t)r.W * r.V * per_lane < N) r.W <<= 1;
    const int G = 64 / r.W;
    if (csr && M > 0) {
        // Dense pattern (mean degree >= 64, >= 4.5 KB gathered per row and slab): cache-blocked form, ~6 MB
        // slabs of D2. The number of D2 rows is not part of the call: the pattern is taken as square for
        // the slab count (columns past M land in the last slab — fewer hits, same result). Needs a
        // stream-ordered temporary for the split points, so not on a stream under capture.
        const int64_t avg_deg = nnz / M;
        int64_t slab_rows = (6 << 20) / (N * es > 0 ? N * es : es);  // 3..6 MB measured best (sddmm_slab.log)
        if (slab_rows < 64) slab_rows = 64;
        const int64_t nslab = (M + slab_rows - 1) / slab_rows;
        // (the edges of a row that fall into one slab must still gather >= ~4.5 KB of D2: with less the per-row
        // overhead of 'nslab' launches outweighs the L2 hits —
        // profiles/r01/sddmm_heuristic_audit.log; M = 10^6, degree 100, 41 slabs was 4.5x slower than streaming)
        if (!capturing && N * es >= 256 && nslab >= 4 && nslab <= 4096 && avg_deg >= 64 &&
            avg_deg * N * es >= 4608 * nslab) {
            r.form = kSddmmBlocked;
            r.nslab = nslab;
            r.slab_rows = slab_rows;
            return r;
        }
        // Long rows but not worth blocking: the same row-walking kernel over the whole row ([rowptr[r], rowptr[r+1])
        // is "one slab") — D1 slice in registers, four edges in flight, no per-edge row search. The edge-parallel
        // form stays for short rows, where a row per wavefront would leave lanes idle.
        if (avg_deg >= kSddmmRowWalkMinDegree) {
            r.form = kSddmmRowWalk;
            return r;
        }
    }
    // edges per wavefront: COO G * UE (UE = 4); CSR 256 — one row search per 256 edges — unless that leaves
    // the chip short of wavefronts (small patterns: pubmed-sized N = 128 ran 18.4 us against COO's 9.8)
    r.epw = G * 4;
    if (csr) r.epw = (nnz >= 256 * 16384) ? 256 : (nnz >= 64 * 16384) ? 64 : (G * 4 > 16 ? G * 4 : 16);
    return r;
}

// The multi-head SDDMM. V, W and the form are resolve_sddmm's at WIDTH F — a head slice is what a lane group walks — so the bits of a
// head are those of the single-head call whatever this function answers. The kernel is taken wherever it can run (H >= 2, pair count
// nnz H within its 32-bit pair arithmetic) — also on CSR patterns of mean degree >= 64, where resolve_sddmm walks rows or blocks: there
// the edge-parallel heads kernel measured 1.8-12x faster than the per-head composition on a skewed and on a uniform dense pattern
// (profiles/r09/sddmm_heads/timing.log). The composition is left with CSR calls past the pair limit, and with the pin.
// Edges per wavefront: the fp32 thresholds of resolve_sddmm applied to the PAIR count nnz H (carried over, not measured on their own)
// give pairs per wavefront — COO G * UE, CSR 256 / 64 / max(G * UE, 16) — and epw is that many pairs in whole edges, 1 .. 256.
// elem_size 2 (fp16 / bf16 operands): V, W and the form are resolve_sddmm's at that element size; route and epw do not look at it.
SddmmHeadsLaunch resolve_sddmm_heads(bool csr, int64_t M, int64_t nnz, int64_t H, int64_t F, int d1_align, int d2_align, bool capturing,
                                     int pin, int elem_size) {
    const SddmmLaunch b = resolve_sddmm(csr, M, nnz, F, d1_align, d2_align, capturing, elem_size);
    SddmmHeadsLaunch r = {kSddmmHeadsComposition, b.form, b.V, b.W, 0, 0};
    if (H == 1) {
        r.route = kSddmmHeadsPlain;
        return r;
    }
    const bool can_run = H >= 2 && F >= 1 && nnz <= kSddmmMaxNnz / H;
    const bool kernel = can_run && (capturing || !(csr && pin == kSddmmHeadsPinComposition));
    if (!kernel) return r;
    r.route = kSddmmHeadsKernel;
    r.form = csr ? kSddmmCsrEdge : kSddmmCooEdge;
    const int64_t pairs = nnz * H;
    const int G = 64 / r.W;
    int64_t per_wave = G * 4;
    if (csr) per_wave = (pairs >= 256 * 16384) ? 256 : (pairs >= 64 * 16384) ? 64 : (G * 4 > 16 ? G * 4 : 16);
    const int64_t epw = per_wave / H;
    r.epw = (int)(epw < 1 ? 1 : (epw > 256 ? 256 : epw));
    // t / H == (t * magic) >> 32 for t < 256 H needs 256 H (magic H - 2^32) < 2^32, and magic H - 2^32 < H: H <= 4096
    if (H <= 4096) r.magic = (uint32_t)(((1ull << 32) + (uint64_t)H - 1) / (uint64_t)H);
    return r;
}

// The edge softmax. A lane group should cover a typical row in one or two steps, so W follows the mean degree alone — up to 16 lanes:
// the starting rule went on to 64, and on products-sbm (mean degree 50.5) W = 64 measured 1.3-2.4x slower than W = 16 at H = 1, 4 and 8,
// forward and backward (a whole wavefront per pair leaves no lane group for the neighbouring heads, so at H > 1 every load instruction
// touches 64 separate words; profiles/r10/edge_softmax/w_cap.log). Rows past kLongRowThreshold take a whole wavefront; that
// value is carried over from the SpMM's long-row pass, not tuned. H only sizes a wavefront's share of rows (about 64 pairs), which no
// result bit depends on.
EdgeSoftmaxLaunch resolve_edge_softmax(int64_t M, int64_t nnz, int64_t H) {
    EdgeSoftmaxLaunch r = {kEdgeSoftmaxMaxW, kLongRowThreshold, 1};
    const int64_t mean = M > 0 ? (nnz + M - 1) / M : kEdgeSoftmaxMaxW;
    int W = 4;
    while (W < kEdgeSoftmaxMaxW && W < mean) W *= 2;
    r.W = W;
    if (H < 64) r.rpw = (int)(64 / (H < 1 ? 1 : H) > 63 ? 63 : 64 / (H < 1 ? 1 : H));
    return r;
}

// The GATv2 score. V and W are resolve_sddmm's at WIDTH F — asked in its COO form, which has no row-walking or blocked answer — with the
// less aligned of xl and xr as one operand and att as the other: V divides F and 4 V bytes divide all THREE bases. Entries per wavefront
// and the multiply-shift for t / H are resolve_sddmm_heads' rule for its CSR kernel, on the pair count nnz H. None of these thresholds
// was measured for this kernel, which loads three vectors per pair where the SDDMM loads two: all are carried over.
static Gatv2ScoreLaunch gatv2_score_launch(const SddmmLaunch& b, int64_t nnz, int64_t H) {
    Gatv2ScoreLaunch r = {b.V, b.W, 0, 0};
    const int64_t pairs = nnz * H;
    const int G = 64 / r.W;
    const int64_t per_wave = (pairs >= 256 * 16384) ? 256 : (pairs >= 64 * 16384) ? 64 : (G * 4 > 16 ? G * 4 : 16);
    const int64_t epw = per_wave / H;
    r.epw = (int)(epw < 1 ? 1 : (epw > 256 ? 256 : epw));
    // t / H == (t * magic) >> 32 for t < 256 H needs 256 H (magic H - 2^32) < 2^32, and magic H - 2^32 < H: H <= 4096
    if (H <= 4096) r.magic = (uint32_t)(((1ull << 32) + (uint64_t)H - 1) / (uint64_t)H);
    return r;
}

Gatv2ScoreLaunch resolve_gatv2_score(int64_t M, int64_t nnz, int64_t H, int64_t F, int xl_align, int xr_align, int att_align) {
    return gatv2_score_launch(resolve_sddmm(false, M, nnz, F, xl_align < xr_align ? xl_align : xr_align, att_align, false, 4), nnz, H);
}

// ... on 16-bit xl and xr (att stays fp32): resolve_sddmm at element size 2 — V counts ELEMENTS, up to 8, and 2 V bytes divide the
// bases of xl and xr. att's V floats are loaded in pieces of at most 16 bytes, so min(4 V, 16) bytes must divide its base: a 16-byte
// aligned att allows every V, an 8-byte aligned one V = 2, a 4-byte aligned one V = 1 — which is the rule "2 V bytes divide" applied to
// half its alignment. W, epw and the multiply-shift as above (carried over, not measured at 16 bits).
Gatv2ScoreLaunch resolve_gatv2_score_x16(int64_t M, int64_t nnz, int64_t H, int64_t F, int xl_align, int xr_align, int att_align) {
    const int att_as_x16 = att_align >= 16 ? 16 : att_align / 2;
    return gatv2_score_launch(resolve_sddmm(false, M, nnz, F, xl_align < xr_align ? xl_align : xr_align, att_as_x16, false, 2), nnz, H);
}

// The fused dot-product attention. V and W are resolve_sddmm's at WIDTH F (its COO form: no row-walking or blocked answer) for the least
// aligned operand: V divides F and 4 V bytes divide every base, W is the smallest power of two in 4 .. 64 with 8 W >= F. The kernels keep
// a head slice in 8 floats per lane, so a slice wider than 8 * 64 floats has no kernel. Nothing here was measured for these kernels.
DotAttentionLaunch resolve_dot_attention(int64_t F, int q_align, int k_align, int v_align) {
    const int kv = k_align < v_align ? k_align : v_align;
    const SddmmLaunch b = resolve_sddmm(false, 1, 1, F, q_align, kv, false, 4);
    return DotAttentionLaunch{b.V, b.W, F <= kDotAttentionMaxF};
}

// ... on 16-bit q, k and v: the fp32 rule at twice each alignment, capped at 16, so that both resolvers answer the same (V, W) for an
// operand and its widened copy placed to match. No V = 8 (a 16-byte load of 16-bit elements): it would move the dot's lane positions.
DotAttentionLaunch resolve_dot_attention_x16(int64_t F, int q_align, int k_align, int v_align) {
    const auto twice = [](int a) { return 2 * a > 16 ? 16 : 2 * a; };
    return resolve_dot_attention(F, twice(q_align), twice(k_align), twice(v_align));
}

// The fused GATv2 attention: the same rule — the one resolve_gatv2_score applies to its three operands — so that on equally aligned
// operands the fused score has the lane positions, hence the bits, of gespmm_gatv2_score_f32. Nothing here was measured for these
// kernels.
Gatv2AttentionLaunch resolve_gatv2_attention(int64_t F, int xl_align, int xr_align, int att_align) {
    const SddmmLaunch b = resolve_sddmm(false, 1, 1, F, xl_align < xr_align ? xl_align : xr_align, att_align, false, 4);
    return Gatv2AttentionLaunch{b.V, b.W, F <= kGatv2AttentionMaxF};
}

// ... on 16-bit node terms: the fp32 rule on the widened operands' alignments, so that both resolvers answer the same (V, W) for an
// operand and its widened copy placed to match. No V = 8 (a 16-byte load of 16-bit elements): it would move the lane positions.
Gatv2AttentionLaunch resolve_gatv2_attention_x16(int64_t F, int xl_align, int xr_align, int att_align) {
    const int l = 2 * xl_align > 16 ? 16 : 2 * xl_align, r = 2 * xr_align > 16 ? 16 : 2 * xr_align;
    return resolve_gatv2_attention(F, l, r, att_align);
}

}  // namespace gespmm
