/*
 * gespmm.h — C ABI of libgespmm.so, the MI355X (gfx950) GE-SpMM hot path.
 *
 * This is the drop-in boundary for the ONE path this repository accelerates:
 * CSR x dense row-product SpMM (fp32 values, int32 indices), plus the SDDMM and
 * CSR->CSC helpers the reference's PyTorch op exposes next to it.
 *
 * Each entry point names the reference interface it replaces (paths relative to
 * the reference repository hgyhungry/ge-spmm):
 *
 *   gespmm_csr_spmm_f32      <- spmmWrapper()                 spmm_test.cu:456-492
 *                               spmm_cuda()                   pytorch-custom/spmm_kernel.cu:425-458
 *                               spmm_cuda_no_edge_value()     pytorch-custom/spmm_kernel.cu:175-207
 *                               XTopoCsrmm<float>()           dgl-custom/binary_reduce_sum.cu:310-335
 *   gespmm_csr_spmm_max_f32  <- XTopoCsrmmmax<float>()        dgl-custom/binary_reduce_max.cu:182-207
 *   gespmm_csr_spmm_max_arg_f32 / gespmm_csr_spmm_max_backward_f32 / gespmm_max_arg_route <- (new) the same reducer with the
 *                               winning CSR position per output word, and the gradient that position gives: what the `pool`
 *                               aggregator of dgl-custom/benchmark/sage/sage_dgl.py needs to train
 *   gespmm_dgl_csrmm_{sum,max}_f32  <- the same two, with exactly their argument lists
 *   gespmm_csr_spmm_workspace_bytes / gespmm_csr_spmm_f32_ws  <- (new) caller-owned scratch, no reference counterpart
 *   gespmm_select_variant    <- the N-based 3-way dispatch    pytorch-custom/spmm_kernel.cu:186-206,437-457
 *   gespmm_sddmm_coo_f32     <- sddmm_cuda_coo()              pytorch-custom/sddmm.cu:427-457
 *   gespmm_sddmm_csr_f32     <- sddmm_cuda_csr()              pytorch-custom/sddmm.cu:459-484
 *   gespmm_csr2csc_f32       <- csr2csc_cuda()/csr2cscKernel  pytorch-custom/spmm_kernel.cu:381-476
 *   gespmm_mtx_read[_cached] / _free  <- readMtx<float>()     util/util.hpp:286-333 (+ mmio.hpp:215,308)
 *   gespmm_coo_to_csr        <- inline COO->CSR               spmm_test.cu:557-581
 *   gespmm_row_partition     <- (new; north_star multi-GPU)   no reference counterpart
 *   gespmm_plan_*            <- (new) analysis stage in front of repeated launches; no reference counterpart
 *   gespmm_init              <- the 200 empty warm-up launches spmm_test.cu:720-721 (same role: start-up cost outside the timed loop)
 *   gespmm_set_auto_plan / gespmm_auto_plan_* <- (new) plans for callers that keep no state: spmmWrapper spmm_test.cu:456-492,
 *                               spmm_cuda spmm_kernel.cu:425-458, CustomCsrmm dgl-custom/binary_reduce_sum.cu:338-360
 *   gespmm_cluster_rows / gespmm_simulate_l2_hits <- (new) the plan's host-side row clustering and its L2 model
 *   gespmm_baseline_atomic_scatter_f32 <- Gunrock app's edge map  gunrock-test/app/spmm/spmm_enactor.cuh:92-105
 *   gespmm_edge_softmax_f32 / _backward_f32 <- (new) softmax over the entries of a CSR row, per head; no reference counterpart
 *   gespmm_gat_softmax_f32 / _backward_f32 / gespmm_edge_segment_sum_f32 <- (new) the same softmax on the additive score of a graph
 *                               attention layer, el[row] + er[col], never written; the per-segment sum of an edge array
 *   gespmm_gat_softmax_stats_f32 / gespmm_gat_aggregate_f32 / gespmm_gat_aggregate_route <- (new) that softmax's row statistics, and the
 *                               multi-head product that computes the attention weights from them: no [nnz x H] array at all
 *   gespmm_gat_backward_el_f32 / gespmm_gat_backward_er_f32 <- (new) the backward of that layer for el and er: two launches on
 *                               node-sized words, no [nnz x H] array either
 *   gespmm_edge_dropout_f32 / gespmm_gat_aggregate_dropout_f32 / gespmm_gat_backward_{el,er}_dropout_f32 / gespmm_edge_dropout_bits /
 *                               _threshold <- (new) dropout on the attention coefficients with a mask that is never stored
 *   gespmm_baseline_copy_f32 <- (new) streaming-copy yardstick for the roofline record; no reference counterpart
 *
 * Conventions (all device entry points):
 *   - every pointer is a DEVICE pointer owned by the caller, except where a
 *     parameter is documented as host memory (the loader / partitioner);
 *   - dense matrices are row-major with leading dimension N (B is K x N, C is M x N);
 *   - C is fully overwritten (alpha = 1, beta = 0, no accumulate, no pre-zeroing);
 *   - the call is asynchronous on `stream` (a hipStream_t passed as void*;
 *     NULL = the legacy default stream, which is what the reference launches on);
 *   - the return value is a hipError_t cast to int (0 = success) or one of the
 *     negative GESPMM_E* codes below; the library never calls exit();
 *   - re-entrant; the only global state is cached, immutable device properties and one memory
 *     pool per device for stream-ordered temporaries (created on first use);
 *   - the device that owns `stream` and the pointers is the calling thread's current device;
 *   - index RANGES are the caller's responsibility, as in the reference: rowptr must be non-decreasing with
 *     rowptr[M] = nnz and every colind entry must lie in [0, K). The device kernels do not check (a check would cost
 *     a pass over the matrix per call); the host-side entry points (loader, COO->CSR, plans) do.
 *
 * There is NO CPU fallback: without a HIP device every compute entry point
 * returns the HIP error (hipErrorNoDevice = 100).
 */
#ifndef GESPMM_H_
#define GESPMM_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GESPMM_VERSION_MAJOR 0
#define GESPMM_VERSION_MINOR 5

/* Negative return codes (positive values are hipError_t). */
#define GESPMM_EINVAL   (-1)  /* bad argument (null pointer, negative size, unknown variant) */
#define GESPMM_EALIGN   (-2)  /* pointer not 4-byte aligned */
#define GESPMM_ERANGE   (-3)  /* size exceeds what int32 CSR indices can address */
#define GESPMM_EIO      (-4)  /* loader: file not found / unreadable */
#define GESPMM_EFORMAT  (-5)  /* loader: bad MatrixMarket banner or size line */
#define GESPMM_ENOMEM   (-6)  /* host allocation failed */
#define GESPMM_ERR_UNSUPPORTED (-7)  /* no kernel serves this shape, and there is no other route (gespmm_dot_attention_f32: F > 512) */

/*
 * Kernel variants. Numbers 0..4 keep the reference's `method` numbering
 * (spmm_test.cu:456-492): 0 naive, 1 CRC, 2/3/4 CRC+CWM with coarsening factor
 * 2/4/8. 5 is the parallel-reduction variant (lanes over nnz) that north_star
 * asks for and the reference only has in dgSPARSE. -1 lets the library choose.
 *
 * Variants 0-4 accumulate each output element in ONE fp32 register in ascending
 * CSR position with one fused multiply-add per non-zero (the arithmetic the
 * reference's device kernels perform); they are bit-identical to each other.
 * Variant 5 changes the summation order and is tolerance-checked.
 *
 * Load balance: in matrices with >= 2^23 non-zeros (or >= 2^20 at mean degree >= 8), rows longer than
 * max(2048, 32 x mean degree) entries (RMAT hubs) are skipped by the main kernel and computed in
 * 2048-entry CHUNKS spread over the whole chip: a workgroup sums one chunk (its lane groups take the
 * chunk's 64-entry tiles round-robin, partial rows added in fixed group order), a combine kernel adds
 * a row's chunk partials in chunk order — bit-reproducible from run to run, but a re-association of
 * the strict chain (within the 1e-4 tolerance, not bit-for-bit). GESPMM_FLAG_STRICT_ORDER (through
 * gespmm_csr_spmm_f32_cfg) keeps every row a strict chain. A gespmm_plan decides from the longest row
 * it actually saw instead of these size rules.
 */
#define GESPMM_VARIANT_AUTO       (-1)
#define GESPMM_VARIANT_NAIVE        0
#define GESPMM_VARIANT_CRC          1
#define GESPMM_VARIANT_CRC_CWM2     2
#define GESPMM_VARIANT_CRC_CWM4     3
#define GESPMM_VARIANT_CRC_CWM8     4
#define GESPMM_VARIANT_PARREDUCE    5
#define GESPMM_NUM_VARIANTS         6

const char* gespmm_version(void);
/* Human-readable string for any return code of this library. */
const char* gespmm_error_string(int code);

/*
 * C[M x N] = A[M x K] * B[K x N], A in CSR (rowptr[M+1], colind[nnz], val[nnz]).
 * val == NULL means A == 1 on its pattern (the "topo"/no_edge_value kernels).
 * nnz may be passed as -1 when unknown (it feeds the variant heuristic and sizes the
 * long-row pass's temporary: with -1 every row keeps the strict chain).
 * Temporaries (dense-graph cache blocking, long-row pass) are stream-ordered allocations
 * from a pool the library owns; on a stream under capture both paths are switched off, so
 * a captured call never allocates.
 */
int gespmm_csr_spmm_f32(const int32_t* rowptr, const int32_t* colind, const float* val,
                        const float* B, float* C,
                        int64_t M, int64_t K, int64_t N, int64_t nnz,
                        int variant, void* stream);

/*
 * Same product with the `max` reducer over the row's neighbours (unweighted):
 * C[r,c] = max_p B[colind[p], c]; rows without non-zeros yield `empty_value`
 * (the reference hard-codes -10000, binary_reduce_max.cu:22-24).
 */
int gespmm_csr_spmm_max_f32(const int32_t* rowptr, const int32_t* colind,
                            const float* B, float* C,
                            int64_t M, int64_t K, int64_t N, int64_t nnz,
                            float empty_value, int variant, void* stream);

/*
 * The max reducer WITH ARGMAX, and its gradient. Forward — one sequential chain per output word (r, c), whatever the lane geometry:
 *
 *     acc = empty_value; a = -1
 *     for p = rowptr[r] .. rowptr[r + 1] - 1, ascending:  b = B[colind[p] N + c];  if (b > acc) { acc = b; a = p; }
 *     C[r, c] = acc;  arg[r, c] = a
 *
 * arg is int32 [M, N] and holds a CSR POSITION, not a column id: repeated (row, column) entries stay distinguishable. Among equal values
 * the smallest position wins; +0 and -0 compare equal, so the first one wins and keeps its sign bit; NaN never wins; a value <=
 * empty_value never wins, and a row that is empty or holds only such values gives (empty_value, -1). C has the bits of
 * gespmm_csr_spmm_max_f32 on every input where no zeros of both signs compete for a maximum (there that entry's fmaxf chain is
 * undefined; this one is not). Every word of C and arg is written.
 *
 * Backward — for node k and column c, over the CSC arrays of the pattern, CSC position q being CSR entry order[q] (what
 * gespmm_csr2csc_f32 gives when csr_val holds the positions; the csc_order of the GAT entries):
 *
 *     g = +0
 *     for q = colptr[k] .. colptr[k + 1] - 1, ascending:  r = rowind[q];  if (arg[r N + c] == order[q]) g = g + grad_out[r N + c]
 *     grad_B[k, c] = g
 *
 * One plain fp32 add chain per output word in CSC order: bit-reproducible, no atomics, no workspace. Every word of grad_B is written,
 * +0 for a node nobody chose. The VALUES of order and arg are trusted (they are compared, never used as an address); rowind must lie
 * in [0, M) as colind in [0, K).
 *
 * One kernel each: the batch-stream walk (a wavefront owns a contiguous range of segments, 64-entry index tiles through LDS, W lanes per
 * segment with V floats per lane) in the geometry gespmm_max_arg_route prints. 32-bit byte offsets and no second route; fp32 only; no
 * plan form; no long-row pass (a hub segment is walked by one lane group). No allocation, no host synchronisation: capturable.
 * Checks, in this order: a negative size, a NaN empty_value -> GESPMM_EINVAL; M, K, N, nnz beyond what gespmm_csr_spmm_f32 takes, or
 * K N 4 >= 2^32 or M N 4 >= 2^32 -> GESPMM_ERANGE; no segment or N == 0 (forward: M == 0, backward: K == 0) -> 0; a NULL operand
 * (colind and B, or rowind, order, arg and grad_out, may be NULL when nnz == 0) -> GESPMM_EINVAL; a pointer not 4-byte aligned ->
 * GESPMM_EALIGN; a result overlapping a dense operand -> GESPMM_EINVAL. nnz == 0 writes every word: (empty_value, -1) or +0. Dense
 * operands that are only 4- or 8-byte aligned, or an N the vector width does not divide, take a narrower vector — same bits.
 */
int gespmm_csr_spmm_max_arg_f32(const int32_t* rowptr, const int32_t* colind, const float* B, float* C, int32_t* arg, int64_t M, int64_t K,
                                int64_t N, int64_t nnz, float empty_value, void* stream);
int gespmm_csr_spmm_max_backward_f32(const int32_t* colptr, const int32_t* rowind, const int32_t* order, const int32_t* arg,
                                     const float* grad_out, float* grad_B, int64_t M, int64_t K, int64_t N, int64_t nnz, void* stream);
/* Host only: the lane geometry of the two calls above as text, "V=.. S=.. W=.." ("form=none" when M == 0 or N == 0), for M segments (the
 * backward: K) of mean length nnz / M at width N. b_align: largest power of two (>= 4) dividing the address of the gathered operands (B;
 * arg and grad_out), c_align: of the results (C and arg; grad_B). Returns the length written or a GESPMM_E* code. */
int gespmm_max_arg_route(int64_t M, int64_t nnz, int64_t N, int b_align, int c_align, char* out, int64_t capacity);

/*
 * The same two on 16-bit dense operands: B [K, N], C [M, N], grad_out [M, N] and grad_B [K, N] are IEEE fp16 or bfloat16 (dtype
 * GESPMM_X16_F16 / GESPMM_X16_BF16, one type per call; anything else -> GESPMM_EINVAL, before every other check); arg stays int32
 * [M, N], empty_value stays a float. A max rounds nothing, so the contract is the fp32 one on the exactly widened operand:
 *
 *     forward    acc = empty_value (fp32, as given); a = -1
 *                for p ascending:  b = widen(B[colind[p] N + c]);  if (b > acc) { acc = b; a = p; }
 *                C[r, c] = narrow(acc);  arg[r, c] = a
 *     backward   g = +0 (fp32);  for q ascending:  if (arg[r N + c] == order[q]) g = g + widen(grad_out[r N + c]);  grad_B[k, c] = narrow(g)
 *
 * widen is exact; narrow rounds ONCE, to nearest even, at the store. C therefore has the bits of narrow(gespmm_csr_spmm_max_arg_f32 on
 * widen(B)) and arg is identical; an empty_value the type cannot hold (-10000 in bf16) is compared exactly and rounded only where a row
 * without a winner stores it. Ties, zeros of both signs and NaN: as above.
 *
 * One kernel each, the fp32 walk with V ELEMENTS per lane: V = 4 needs 8-byte aligned 16-bit arrays and a 16-byte aligned arg, V = 2
 * 4- and 8-byte, V = 1 serves any N and any 2-byte aligned address (2-byte loads and stores; no composition route, no scratch). 16-byte
 * loads (V = 8) are not built. Checks and their order are those of the fp32 entries; the 16-bit arrays must be 2-byte aligned (index
 * arrays and arg: 4), overlaps count 2 bytes per 16-bit element, and the size limits are unchanged — K N 4 < 2^32 and M N 4 < 2^32 —
 * because arg is the 4-byte array that sets them. No allocation, no host synchronisation: capturable.
 */
int gespmm_csr_spmm_max_arg_x16(const int32_t* rowptr, const int32_t* colind, const void* B, void* C, int32_t* arg, int64_t M, int64_t K,
                                int64_t N, int64_t nnz, float empty_value, int dtype, void* stream);
int gespmm_csr_spmm_max_backward_x16(const int32_t* colptr, const int32_t* rowind, const int32_t* order, const int32_t* arg,
                                     const void* grad_out, void* grad_B, int64_t M, int64_t K, int64_t N, int64_t nnz, int dtype,
                                     void* stream);
/* Host only: gespmm_max_arg_route for the two calls above, V in ELEMENTS. x16_align: largest power of two (>= 2) dividing the addresses
 * of the 16-bit arrays, arg_align: (>= 4) of arg. The answer is gespmm_max_arg_route's at the alignment min(2 x16_align, arg_align). */
int gespmm_max_arg_route_x16(int64_t M, int64_t nnz, int64_t N, int x16_align, int arg_align, char* out, int64_t capacity);

/* The variant `GESPMM_VARIANT_AUTO` resolves to for this shape (pure host logic). */
int gespmm_select_variant(int64_t M, int64_t nnz, int64_t N);

/*
 * Explicit launch geometry, for tuning sweeps and tests. Fields set to 0 mean
 * "library default for this variant and N".
 *   vec      floats per lane per strip (1, 2 or 4) — contiguous, one vector load
 *   strips   strips per lane (1 or 2); coarsening factor = vec * strips
 *   group    lanes cooperating on one row (4..64, power of two); a 64-lane
 *            wavefront therefore carries 64/group rows
 *   rows_per_wave  consecutive rows one lane group streams through (1..32). With
 *            GESPMM_FLAG_BATCH_STREAM: rows per wavefront (rounded to a multiple of 64/group)
 *   flags    GESPMM_FLAG_* bits
 */
typedef struct gespmm_launch_cfg {
    int32_t vec;
    int32_t strips;
    int32_t group;
    int32_t rows_per_wave;
    int32_t slab_rows;   /* cache-blocked path: B rows per column slab (0 = ~6 MB worth) */
    int32_t flags;
} gespmm_launch_cfg;

#define GESPMM_FLAG_NO_XCD_REMAP   0x1  /* plain blockIdx -> row-block mapping */
#define GESPMM_FLAG_NT_STORE       0x2  /* non-temporal stores of C */
#define GESPMM_FLAG_SC1_STORE      0x8000 /* streaming kernels: C stored with system scope (written through instead of kept in the
                                            XCD's L2). Neutral where B exceeds the L2s; with B L2-resident and C not, +20 % when the
                                            reuse of B is skewed, -13 % when it is uniform (profiles/r02/l2_resident_store_scope.log).
                                            The cache-blocked path always stores this way */
#define GESPMM_FLAG_FORCE_IDX64    0x4  /* 64-bit B offsets even when K*N*4 < 2^32 */
#define GESPMM_FLAG_SHALLOW_UNROLL 0x10 /* gather 4 instead of 8 B rows per step (fewer VGPRs) */
#define GESPMM_FLAG_BATCH_STREAM   0x20 /* force the batch-stream kernel (rows walked 64/group at a time) */
#define GESPMM_FLAG_STRICT_ORDER   0x100 /* never split long rows: every row is one strict CSR-order chain */
#define GESPMM_FLAG_SPLIT_LONG_ROWS 0x200 /* run the long-row pass regardless of matrix size */
#define GESPMM_FLAG_SLAB_BLOCKED   0x400 /* force the cache-blocked path (one launch per column slab of B) */
#define GESPMM_FLAG_NO_SLAB_BLOCKED 0x800 /* never use it */
#define GESPMM_FLAG_REUSE_SPLIT     0x2000 /* gespmm_csr_spmm_f32_ws only: `workspace` already holds the split points an earlier call
                                             wrote for the SAME rowptr/colind/N/cfg (cache-blocked path): skip the scan. The caller
                                             vouches that the graph did not change; ignored on every other path */
#define GESPMM_FLAG_ALLOW_REASSOCIATION 0x1000 /* AUTO may pick the parallel-reduction variant (N <= 16, dense rows) */
#define GESPMM_FLAG_SEG_STREAM     0x80 /* force the segmented-stream kernel (AUTO takes it for short rows over an L2-resident B and
                                           for mean degree <= 3; ignored where long rows are split) */

int gespmm_csr_spmm_f32_cfg(const int32_t* rowptr, const int32_t* colind, const float* val,
                            const float* B, float* C,
                            int64_t M, int64_t K, int64_t N, int64_t nnz,
                            int variant, const gespmm_launch_cfg* cfg, void* stream);

/*
 * The same product with a CALLER-PROVIDED temporary (cuSPARSE/rocSPARSE style: query, allocate,
 * run). Two paths of the library need scratch memory — column-slab cache blocking for dense
 * graphs (per-row split points) and the chunked long-row pass (partial rows). The plain entry
 * points above take it stream-ordered from a pool the library owns; this one uses
 * `workspace` (device memory, 16-byte aligned, at least gespmm_csr_spmm_workspace_bytes() for
 * the same shape/variant/cfg) and never allocates — which also keeps both paths available on a
 * stream that is being captured into a HIP graph. workspace_bytes == 0 behaves like
 * gespmm_csr_spmm_f32_cfg. A framework binding passes memory from the framework's own
 * caching allocator here.
 */
int64_t gespmm_csr_spmm_workspace_bytes(int64_t M, int64_t K, int64_t N, int64_t nnz, int variant,
                                        const gespmm_launch_cfg* cfg /* may be NULL */);
int gespmm_csr_spmm_f32_ws(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B, float* C,
                           int64_t M, int64_t K, int64_t N, int64_t nnz, int variant,
                           const gespmm_launch_cfg* cfg /* may be NULL */, void* workspace, int64_t workspace_bytes,
                           void* stream);

/*
 * What a call with these arguments would launch, as one line of text (host-only; no device work): kernel
 * family, vector width V, strips S, lanes per row W, task size, and for the two special paths the slab /
 * long-row parameters — e.g. "variant=3 kernel=batch-stream V=4 S=1 W=32 rows_per_wave=4 idx32" or
 * "variant=3 kernel=slab-blocked V=4 S=1 W=32 slab_rows=12288 slabs=19 idx32". B and C are assumed
 * 16-byte aligned. Returns the length written (excluding the NUL), or a negative code.
 */
int gespmm_describe_launch(int64_t M, int64_t K, int64_t N, int64_t nnz, int variant,
                           const gespmm_launch_cfg* cfg /* may be NULL */, char* out, int64_t capacity);


/*
 * The DGL kernel patch's entry points (dgl-custom/binary_reduce_sum.cu:310-335 XTopoCsrmm<float>,
 * binary_reduce_max.cu:182-207 XTopoCsrmmmax<float>) with their argument list — (m, n, indptr,
 * indices, B, C) plus the stream DGL keeps in its RuntimeConfig: C[m x n] = sum / max over the
 * row's neighbours of B[neighbour, :], A == 1 on the CSR pattern. DGL passes neither the number
 * of source nodes nor nnz at that point: 64-bit offsets into B are used; for graphs of 32768 rows
 * or more nnz is read back from indptr[m] (a stream synchronisation, as the patch does after its
 * kernel) so that dense graphs and hub rows get their dedicated paths, smaller graphs keep the
 * strict CSR-order chain for every row. Rows without neighbours give 0 (sum) or -10000 (max: the patch's
 * max_init, binary_reduce_max.cu:22-24). Returns 0 or an error code as above (the patch returns
 * its cudaError the same way).
 * The read-back is a policy, not part of the product: gespmm_dgl_set_readback_rows(rows) moves the threshold
 * (process-wide; rows < 0 = never synchronise: every call is then fully asynchronous and every row a strict chain;
 * 0 = always). On a stream under capture the entry points never read back, whatever the threshold.
 */
int gespmm_dgl_set_readback_rows(int64_t rows);
int gespmm_dgl_csrmm_sum_f32(int m, int n, const int32_t* indptr, const int32_t* indices, const float* B, float* C,
                             void* stream);
int gespmm_dgl_csrmm_max_f32(int m, int n, const int32_t* indptr, const int32_t* indices, const float* B, float* C,
                             void* stream);

/*
 * SDDMM: out[e] = sum_j D1[row(e), j] * D2[col(e), j], e in pattern order.
 * COO: row(e) = rowind[e].  CSR: row(e) = the row whose [rowptr[r], rowptr[r+1]) holds e.
 * D1 is M x N, D2 is K x N, row-major; out has nnz floats (N == 0: zeros).
 * nnz <= 2^31 - 1 - 4096 (GESPMM_ERANGE beyond: the kernels count edges in 32 bits, a wavefront's span past the end included).
 * Summation order: W lanes share an edge, each loads V floats at a time. Lane l runs ONE fmaf chain, from 0, over the elements
 * j = l*V + t*W*V + i (t ascending; i = 0..V-1 ascending; j < N); then for m = W/2, W/4, .. 1 every lane adds the partial sum
 * of lane l ^ m to its own; lane 0's sum is out[e]. V is the widest of 4, 2, 1 that divides N and whose 4*V bytes divide both
 * operand addresses; W the smallest power of two in 4..64 with W * V * (2, 4, 8 for V = 4, 2, 1) >= N (64 beyond). The order
 * depends on nothing else — not on the form (COO, CSR, a plan), the pattern, or the launch the library picks.
 */
int gespmm_sddmm_coo_f32(const int32_t* rowind, const int32_t* colind,
                         const float* D1, const float* D2, float* out,
                         int64_t nnz, int64_t N, void* stream);
int gespmm_sddmm_csr_f32(const int32_t* rowptr, const int32_t* colind,
                         const float* D1, const float* D2, float* out,
                         int64_t M, int64_t nnz, int64_t N, void* stream);

/*
 * What an SDDMM call with these arguments would launch, as one line of text (since 0.5; host-only, no device work), in the
 * manner of gespmm_describe_launch: "form=coo-edge V=4 W=32 epw=8", "form=csr-edge V=1 W=64 epw=256" (epw: edges per
 * wavefront), "form=row-walk V=4 W=32" (a row per wavefront, mean degree >= 64), "form=blocked V=1 W=64 nslab=5
 * slab_rows=3066" (the row walk once per ~6 MB column slab of D2; allocates, so never with capturing != 0), "form=none"
 * (nnz == 0). csr: 0 = gespmm_sddmm_coo_f32 (M is ignored), else gespmm_sddmm_csr_f32. d1_align / d2_align: a power of
 * two >= 4 that divides the operand's address (16 = as good as it gets). Returns the length written or a negative code.
 */
int gespmm_describe_sddmm(int csr, int64_t M, int64_t nnz, int64_t N, int d1_align, int d2_align, int capturing,
                          char* out, int64_t capacity);

/*
 * SDDMM on 16-bit dense operands (same ABI version): out[e] = sum_j D1[row(e), j] * D2[col(e), j] with D1 [M x N] and D2 [K x N]
 * row-major IEEE fp16 (GESPMM_X16_F16) or bfloat16 (GESPMM_X16_BF16), both of the same type; out[nnz] is FP32 and is not narrowed
 * (edge values are fp32 everywhere in this library: out feeds the `val` of the products directly). Every element is widened
 * exactly (subnormals included) and the sum is the lane formula above in fp32: per edge W lanes each run ONE fmaf chain, from 0,
 * over the elements j = l*V + t*W*V + i, then the xor butterfly over masks W/2 .. 1, lane 0's sum is out[e]. No dot2 and no
 * packed-fp16 arithmetic. The product of two fp16 or two bf16 numbers is exact in fp32, so the result depends on (V, W) alone, and
 * V counts ELEMENTS here: the widest of 8, 4, 2, 1 that divides N and whose 2*V bytes divide both operand addresses; W the smallest
 * power of two in 4..64 with W * V * (2, 4, 8, 8 for V = 8, 4, 2, 1) >= N (64 beyond). This is the fp32 geometry at half the byte
 * width — N = 128 is (8, 8), not the fp32 call's (4, 16) — so the order, and with it the last bits, DIFFER from
 * gespmm_sddmm_*_f32 on the widened operands wherever (V, W) differ: SDDMM's order is pinned by the formula, not by the fp32 call.
 * Every N and every 2-byte aligned address runs a 16-bit kernel (there is no widening pass and no temporary beyond the blocked
 * form's split points); the forms and their thresholds are those of the fp32 calls with the row bytes taken as 2 N. Checks, in
 * the order of the fp32 entry points and before any device work: negative sizes or a dtype other than the two -> GESPMM_EINVAL;
 * sizes out of range -> GESPMM_ERANGE; nnz == 0 -> 0; NULL pointers -> GESPMM_EINVAL; D1 / D2 off a 2-byte boundary (index
 * arrays and out: 4-byte) -> GESPMM_EALIGN. gespmm_describe_sddmm_x16: as gespmm_describe_sddmm, alignments powers of two >= 2.
 * (GESPMM_X16_F16 = 1, GESPMM_X16_BF16 = 2: defined with gespmm_csr_spmm_x16 below.)
 */
int gespmm_sddmm_coo_x16(const int32_t* rowind, const int32_t* colind, const void* D1, const void* D2, float* out,
                         int dtype, int64_t nnz, int64_t N, void* stream);
int gespmm_sddmm_csr_x16(const int32_t* rowptr, const int32_t* colind, const void* D1, const void* D2, float* out,
                         int dtype, int64_t M, int64_t nnz, int64_t N, void* stream);
int gespmm_describe_sddmm_x16(int csr, int64_t M, int64_t nnz, int64_t N, int d1_align, int d2_align, int capturing,
                              char* out, int64_t capacity);

/*
 * CSR (M x K) -> CSC on the device: fills colptr[K+1], rowind[nnz] and, when
 * csr_val != NULL, csc_val[nnz]. Entries inside one column keep ascending row
 * order (stable), which is what makes backward SpMM on the CSC arrays
 * deterministic. `workspace` must hold gespmm_csr2csc_workspace_bytes() bytes.
 */
int64_t gespmm_csr2csc_workspace_bytes(int64_t M, int64_t K, int64_t nnz);
int gespmm_csr2csc_f32(const int32_t* rowptr, const int32_t* colind, const float* csr_val,
                       int32_t* colptr, int32_t* rowind, float* csc_val,
                       int64_t M, int64_t K, int64_t nnz,
                       void* workspace, void* stream);

/*
 * ------------------------------------------------------------------ plans (analysis stage)
 *
 * Repeated products with ONE sparse matrix (200 timed launches in spmm_test.cu:754-762; every layer of every
 * epoch in gcn_custom.py:118-143) can be prepared once. The reference has no such stage — its kernels walk the
 * rows in storage order on every launch; vendor SpMMs have one (rocsparse_spmm_stage_preprocess). A plan
 *   - reads the matrix ONCE, on the device (validation, clustering, L2 model, task cutting are device passes;
 *     gespmm_plan_create synchronises `stream` a handful of times; GESPMM_PLAN_ANALYSIS_HOST keeps the host form),
 *   - decides the long-row pass from the longest row it actually saw,
 *   - keeps the scratch of the cache-blocked path (dense graphs) so its split scan runs once,
 *   - and, for sparse graphs whose B exceeds the L2s, keeps a ROW-CLUSTERED copy of the matrix plus a task
 *     table with an equal non-zero budget per wavefront: rows that share neighbours are processed next to each
 *     other, so the B rows they share come from the XCD's L2 instead of crossing the fabric again.
 * The order in which rows are PROCESSED is the only thing a plan changes: each row is still one fp32 chain in
 * its own CSR order written to its own row of C, so gespmm_plan_spmm_f32 returns the same bits as
 * gespmm_csr_spmm_f32: the long-row pass (a re-association of rows beyond 32x the mean degree / 2048 entries) runs under a
 * plan exactly where the plain call runs it — matrices of >= 2^23 non-zeros, or >= 2^20 with mean degree >= 8 — and, because
 * the plan has SEEN the longest row, only when such a row exists. GESPMM_FLAG_SPLIT_LONG_ROWS / _STRICT_ORDER in
 * gespmm_plan_options.flags force it on / off (as they do for the plain call).
 *
 * rowptr / colind / val are DEVICE pointers. A plan that keeps the storage order (small or dense matrices, or
 * reorder = GESPMM_PLAN_NO_REORDER) keeps referring to them, so they must outlive the plan; a clustered plan owns
 * copies. After changing the VALUES call gespmm_plan_set_values; a changed pattern needs a new plan.
 * One plan serves one stream at a time.
 */
typedef struct gespmm_plan gespmm_plan;

#define GESPMM_PLAN_REORDER_AUTO 0  /* cluster when B exceeds the L2s and the model of the L2s predicts a gain */
#define GESPMM_PLAN_REORDER      1  /* always cluster (streaming-kernel family only) */
#define GESPMM_PLAN_NO_REORDER   2  /* keep the storage order */

typedef struct gespmm_plan_options {
    int32_t reorder;       /* GESPMM_PLAN_REORDER_* */
    int32_t task_entries;  /* work per wavefront task of a clustered plan in non-zeros, 0 = default for N */
    int32_t row_floor;     /* a row counts as at least this many non-zeros when tasks are cut (the kernel spends one
                              memory round trip per row pair however short the rows are), 0 = default, -1 = none */
    int32_t threads;       /* host threads for the clustering, 0 = all (the result does not depend on it) */
    int32_t flags;         /* GESPMM_FLAG_* applied to every launch (e.g. GESPMM_FLAG_STRICT_ORDER) */
    int32_t kernel;        /* GESPMM_PLAN_KERNEL_*: which kernel a clustered plan launches */
    int32_t analysis;      /* GESPMM_PLAN_ANALYSIS_*: where the clustering / L2 model / task cutting run (since 0.2) */
    int32_t expected_launches; /* products this plan is expected to serve, 0 = 200 (the reference's ITER, spmm_test.cu:714; its GCN runs 200
                              epochs, gcn_custom.py:134). reorder = AUTO weighs the analysis against them: clustering is skipped when the
                              estimated gain per launch x launches does not pay for its estimated time, and plans with launches x N < 100 000
                              cluster three levels deep instead of six (since 0.3, gespmm_plan_create_v2 only) */
} gespmm_plan_options;
/*
 * Plan options and versions. Every field's default is 0 and fields are only ever APPENDED. gespmm_plan_create is the
 * un-versioned symbol: it reads the SEVEN fields every header that shipped with it alone had (reorder .. analysis) and nothing
 * beyond them, whatever header the caller was built with. gespmm_plan_create_v2 takes sizeof(gespmm_plan_options) as the caller's compiler saw it (`opt_bytes`): fields the
 * caller does not have take their defaults, bytes this library does not know are ignored.
 */

#define GESPMM_PLAN_ANALYSIS_DEVICE 0  /* on the device (default): no copy of the matrix leaves HBM */
#define GESPMM_PLAN_ANALYSIS_HOST   1  /* round-2 path: the matrix is copied to the host and clustered there (same order) */

#define GESPMM_PLAN_KERNEL_AUTO     0  /* batch-stream kernel on the task table; segmented-stream for products-shaped rows */
#define GESPMM_PLAN_KERNEL_STREAM   1  /* batch-stream kernel on the task table */
#define GESPMM_PLAN_KERNEL_SEG_STREAM 3 /* segmented-stream kernel on a task table per lane group */
/* (values 2 and 4 belonged to two opt-in kernels of rounds 2-3 — LDS-staged task rows, task-outer — that never beat the
   streaming kernels; their sources and logs are under profiles/r02/experiments/. gespmm_plan_create answers GESPMM_EINVAL.) */
#define GESPMM_PLAN_KERNEL_STAGED 5     /* scalar-stream walk + the most used B rows of every block of 96 / 64 clustered rows staged in LDS
                                          (N = 128, 256, 512 or 1024 — 256-column tiles bound to XCDs beyond 256; sum reducer, device
                                          analysis; rows beyond 2048 entries go to the long-row pass). AUTO takes it for clustered
                                          matrices with mean degree >= 12 (N = 128) / >= 5 (wider) when >= 60 % (N = 128) / 42 % of
                                          the entries find their B row staged (csrc/plan_policy.cpp: hold-out audit). With
                                          reorder = GESPMM_PLAN_NO_REORDER the plan copies the matrix in the caller's order and builds the
                                          tables on that (a matrix that arrives clustered). On square matrices slots a block leaves free
                                          go to single-use columns of near rows (the fill pass: GESPMM_STAGED_FILL) */
#define GESPMM_PLAN_KERNEL_RECORDS 6    /* padded-record kernel (since 0.3, round 6): 4 <= N <= 64, rows of <= 1024 entries, sum reducer,
                                          max(M, K) * N * 4 < 4 GB — the plan lays its copy of the matrix out as batches of 8-slot row pieces
                                          (one coalesced load per lane, all 8 gathers of a piece in flight at once); AUTO takes it for short
                                          rows at narrow widths; other launches of the plan fall back to the streaming kernels */

#define GESPMM_PLAN_KERNEL_STAGED_SLABS 7 /* (since 0.3, round 6) the staged-rows kernel over P ascending COLUMN ranges of the clustered matrix, one
                                          staging list per (block of rows, range) and one launch per range, the second and later ones continuing
                                          from the partial sums in C — for dense clustered matrices (a reddit-shaped community refers to ~100 000
                                          B rows; 160 LDS slots per block cover a seventh of its entries, per range two thirds). N = 128, sum
                                          reducer, rows with non-decreasing columns (range order == CSR order: the same bits), no slab of a row
                                          beyond 2048 entries — else the plan keeps its other kernels. AUTO takes it at mean degree >= 96 when
                                          >= 50 % of the entries find their B row staged */

int gespmm_plan_create(gespmm_plan** plan, const int32_t* rowptr, const int32_t* colind, const float* val /* may be NULL */,
                       int64_t M, int64_t K, int64_t nnz, int64_t N /* width the plan is tuned for */, int variant,
                       const gespmm_plan_options* opt /* may be NULL */, void* stream);
int gespmm_plan_create_v2(gespmm_plan** plan, const int32_t* rowptr, const int32_t* colind, const float* val, int64_t M,
                          int64_t K, int64_t nnz, int64_t N, int variant, const gespmm_plan_options* opt /* may be NULL */,
                          int64_t opt_bytes /* sizeof(gespmm_plan_options) in the caller */, void* stream);
/* C[M x N] = A * B through the plan; any N is legal (scratch and task size are tuned for the plan's N). */
int gespmm_plan_spmm_f32(gespmm_plan* plan, const float* B, float* C, int64_t N, void* stream);
/*
 * The fused product (since 0.4): C = D_r (A (D_c B)) + 1 bias^T with three optional DEVICE vectors col_scale[K], row_scale[M],
 * bias[N] — the normalisation a graph convolution wraps around its SpMM (pytorch-custom/op.py:141-147), without the three
 * elementwise passes over an M x N matrix:
 *
 *     b'(k,c)  = fl32( B[k,c] * col_scale[k] )                 (col_scale == NULL: b' = B)
 *     acc(r,c) = fma(val[p], b'(colind[p],c), acc) over the row's entries in CSR order, acc0 = 0   (val == NULL: acc + b')
 *     t(r,c)   = fl32( acc(r,c) * row_scale[r] )               (row_scale == NULL: t = acc)
 *     C[r,c]   = fl32( t(r,c) + bias[c] )                      (bias == NULL: C = t)
 *
 * Every fl32 is one round-to-nearest operation: the multiply and the add are never contracted and a scale is never folded into
 * `val`. That is the arithmetic of `mul`, gespmm_csr_spmm_f32, `mul`, `add` as separate passes, so the result has THE SAME BITS as
 * that composition — rows without entries (0 * row_scale + bias) and infinite scales (0 * inf = NaN) included. With all three
 * vectors NULL the calls are gespmm_csr_spmm_f32 / gespmm_plan_spmm_f32. Sum reducer only.
 *
 * Two executions, same bits: ONE fused streaming kernel where the unfused launch would be one streaming kernel (batch-stream or
 * segmented-stream, on the caller's arrays or on a clustered plan's task tables; 32-bit offsets, no long-row pass, no cache
 * blocking), else the composition — col_scale . B into a temporary, the unfused launch unchanged, an in-place epilogue. The
 * stateless call takes the K x N temporary stream-ordered from the library's pool; a plan owns it (allocated by the first fused
 * call that needs it, freed with the plan). On a capturing stream a composition that would have to allocate returns
 * hipErrorStreamCaptureUnsupported and launches nothing; a plan whose temporary exists captures fine.
 * Conventions as everywhere in this header: device pointers, asynchronous on `stream`, GESPMM_EINVAL / GESPMM_EALIGN checked
 * before any device work.
 */
int gespmm_csr_spmm_fused_f32(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B,
                              const float* col_scale, const float* row_scale, const float* bias, float* C,
                              int64_t M, int64_t K, int64_t N, int64_t nnz, int variant, void* stream);
int gespmm_plan_spmm_fused_f32(gespmm_plan* plan, const float* B, const float* col_scale, const float* row_scale,
                               const float* bias, float* C, int64_t N, void* stream);
/* host only: what the call above would do at width N with these vectors present (operands on 16-byte boundaries).
   0 composition, 1 fused batch-stream, 2 fused segmented-stream */
int gespmm_plan_fused_route(const gespmm_plan* plan, int64_t N, int has_col_scale, int has_row_scale, int has_bias);
/*
 * 16-bit dense operands: C = A * B with B [K x N] and C [M x N] row-major arrays of IEEE fp16 (GESPMM_X16_F16) or bfloat16
 * (GESPMM_X16_BF16); `val` stays fp32 (or NULL: A == 1 on its pattern). The sum is fp32 and is rounded ONCE:
 *
 *     b(k,c)   = widen(B[k,c])                         exact: every fp16 / bf16 value is an fp32 value, subnormals included
 *     acc(r,c) = fma(val[p], b(colind[p],c), acc) over the row's entries in CSR order, acc0 = 0   (val == NULL: acc + b)
 *     C[r,c]   = narrow(acc(r,c))                      one round-to-nearest-even fp32 -> 16 bits
 *
 * Overflow gives +-inf, a result that is subnormal in the 16-bit type is rounded (not flushed), NaN stays NaN (payload not pinned).
 * For bf16, narrow of a non-NaN with fp32 bits u is (u + 0x7fff + ((u >> 16) & 1)) >> 16. The sum is never held in 16 bits. So the
 * result has THE SAME BITS as widen, gespmm_csr_spmm_f32 / gespmm_plan_spmm_f32, narrow as separate passes; where that fp32 call
 * re-associates (long-row pass) the 16-bit call re-associates identically.
 *
 * Two executions, same bits: ONE 16-bit streaming kernel (batch-stream or segmented-stream, on the caller's arrays or on a
 * clustered plan's task tables) where N is even, B and C are 4-byte aligned (8 and 16 bytes allow wider accesses) and the fp32 call
 * of the byte-equivalent width N / 2 would be one streaming kernel with 32-bit offsets (K N 2 < 2^32; no long-row pass, no cache
 * blocking); else the composition — widen B into a K x N fp32 temporary, the unchanged fp32 route into an M x N one, narrow into C.
 * The stateless call takes both temporaries stream-ordered from the library's pool; a plan owns them (allocated by the first call
 * that needs them, freed with the plan). On a capturing stream a composition that would have to allocate returns
 * hipErrorStreamCaptureUnsupported and launches nothing; a plan whose temporaries exist captures fine.
 * The stateless entry does NOT take part in gespmm_set_auto_plan. gespmm_plan_describe names the route the last 16-bit call took.
 * Conventions as everywhere in this header: device pointers, asynchronous on `stream`; GESPMM_EINVAL (unknown dtype, NULL pointers,
 * negative sizes, bad variant) and GESPMM_EALIGN (B or C not 2-byte aligned, val not 4-byte aligned) are checked before any device
 * work; M == 0 or N == 0 returns 0.
 */
#define GESPMM_X16_F16  1
#define GESPMM_X16_BF16 2
int gespmm_csr_spmm_x16(const int32_t* rowptr, const int32_t* colind, const float* val, const void* B, void* C, int dtype,
                        int64_t M, int64_t K, int64_t N, int64_t nnz, int variant, void* stream);
int gespmm_plan_spmm_x16(gespmm_plan* plan, const void* B, void* C, int dtype, int64_t N, void* stream);
/* host only: what the calls above would do with operands whose addresses b_align / c_align (powers of two) divide, on a stream that
   is not capturing. 0 composition, 1 16-bit batch-stream kernel, 2 16-bit segmented-stream kernel */
int gespmm_x16_route(int64_t M, int64_t K, int64_t N, int64_t nnz, int variant, int b_align, int c_align);
int gespmm_plan_x16_route(const gespmm_plan* plan, int64_t N, int b_align, int c_align);
/*
 * Multi-head product: H weights per edge (attention layers). `val` is row-major [nnz, H], B is [K x H F] and C is [M x H F], fp32,
 * contiguous, N = H F:
 *
 *     C[r, h F + f] = acc,  acc0 = 0,  acc = fmaf(val[p H + h], B[colind[p] N + h F + f], acc) over the row's entries p in CSR order
 *
 * ONE fp32 chain per output element in strict CSR order, never re-associated whatever the matrix size: head h has THE SAME BITS as
 * gespmm_csr_spmm_f32_cfg with GESPMM_FLAG_STRICT_ORDER on the contiguous copies val[:, h] and B[:, h F : (h + 1) F].
 *
 * Two executions, same bits: route 1, ONE heads kernel (the batch-stream kernel at width N with the H weights of every staged entry
 * in LDS; on the caller's arrays or on a clustered plan's task table) where 2 <= H <= 8 and offsets are 32-bit (K N 4 < 2^32,
 * nnz H < 2^31); else route 0, the composition — per head, gather its weights and its slice of B into stream-ordered temporaries from
 * the library's pool, the strict-order product, scatter into C (H = 1: that product on the caller's arrays, no temporaries). On a
 * capturing stream a composition that would have to allocate returns hipErrorStreamCaptureUnsupported and launches nothing.
 * Through a plan the weights are an argument of every call, in the CALLER's edge order; nothing is cached between calls and the plan's
 * own values (gespmm_plan_set_values) are not touched. A clustered plan permutes them into a plan-owned buffer first (one copy kernel
 * per call; the buffer is allocated by the first call and again when H grows — never on a capturing stream).
 * A matrix without entries (nnz == 0; val, colind and B may then be NULL) gives C = 0 on either route.
 * The environment variable GESPMM_HEADS_ROUTE=composition pins route 0 (a measurement knob, read with getenv on every call and route
 * query: do not change the environment from another thread while calls are in flight).
 * The max reducer and the fused vectors have no multi-head entry; 16-bit B and C have one of their own, gespmm_csr_spmm_heads_x16
 * below (stateless only). Not part of gespmm_set_auto_plan.
 * GESPMM_EINVAL (H < 1, negative sizes, NULL pointers), GESPMM_EALIGN (a pointer not 4-byte aligned) and GESPMM_ERANGE (H F or nnz
 * beyond what the other entries take) are checked before any device work; M == 0 or H F == 0 returns 0 without looking at pointers.
 */
int gespmm_csr_spmm_heads_f32(const int32_t* rowptr, const int32_t* colind, const float* val, const float* B, float* C,
                              int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, void* stream);
int gespmm_plan_spmm_heads_f32(gespmm_plan* plan, const float* val, const float* B, float* C, int64_t H, int64_t F, void* stream);
/* host only: the route of the calls above (0 / 1, or GESPMM_E*) for operands whose addresses b_align / c_align (powers of two) divide.
   geometry_out: NULL or int32[4] — V, S, W and rows per wavefront of the kernel (zeros on route 0) */
int gespmm_heads_route(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, int b_align, int c_align, int32_t* geometry_out);
int gespmm_plan_heads_route(const gespmm_plan* plan, int64_t H, int64_t F, int b_align, int c_align);
/*
 * The multi-head product on 16-bit dense operands (since 0.5): B [K x H F] and C [M x H F] hold IEEE fp16 or bfloat16 (dtype:
 * GESPMM_X16_F16 / GESPMM_X16_BF16, both the same), val stays fp32 [nnz x H] — edge-sized arrays are fp32 everywhere in this library.
 * C has the bits of narrow(gespmm_csr_spmm_heads_f32(val, widen(B))): every output element is one fp32 fmaf chain in strict CSR order,
 * never re-associated and never held in 16 bits, rounded ONCE, to nearest even, at the store (overflow gives +-inf, NaN stays NaN);
 * widening is exact, fp16 subnormals included.
 * Routes (gespmm_heads_x16_route): 1 = ONE kernel, the multi-head batch-stream kernel working in 32-bit words (two elements each, both
 * under the staged weight of their head): 2 <= H <= 8, F even, B and C 4-byte aligned (8 / 16 bytes allow wider vectors), 32-bit
 * offsets (K H F 2 < 2^32, nnz H < 2^31) and a lane geometry of gespmm_heads_route's list resolved for the width in words, H F / 2,
 * with V | F / 2; no workspace, no allocation: capturable. 0 = the composition — everything else: H = 1, H > 8, odd F, operands that are
 * only 2-byte aligned, 64-bit offsets: B widened into a stream-ordered temporary from the library's pool, gespmm_csr_spmm_heads_f32
 * into a second one, narrowed into C; the same bits; on a capturing stream it returns hipErrorStreamCaptureUnsupported and launches
 * nothing. GESPMM_HEADS_X16_ROUTE=composition pins route 0 (a measurement knob, read with getenv on every call and route query).
 * There is no plan form: a clustered plan's per-call permutation of the weights costs more than its order gains for this product.
 * Checks before any device work: an unknown dtype, H < 1, negative sizes -> GESPMM_EINVAL; sizes beyond what the fp32 entry takes ->
 * GESPMM_ERANGE; M == 0 or H F == 0 -> 0 without looking at pointers; NULL pointers -> GESPMM_EINVAL; B or C not 2-byte aligned, val,
 * rowptr or colind not 4-byte aligned -> GESPMM_EALIGN. nnz == 0 (val, colind and B may then be NULL) gives C = all-zero bits on
 * either route.
 */
int gespmm_csr_spmm_heads_x16(const int32_t* rowptr, const int32_t* colind, const float* val, const void* B, void* C, int dtype,
                              int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, void* stream);
/* host only: the route of the call above (0 / 1, or GESPMM_E*), as gespmm_heads_route; geometry_out: V (in 32-bit words), S, W and rows
   per wavefront of the kernel (zeros on route 0) */
int gespmm_heads_x16_route(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, int b_align, int c_align, int32_t* geometry_out);
/*
 * The multi-head product with its weights read THROUGH AN EDGE ORDER (since 0.5): order is int32 [nnz] with entries in [0, nnz) (not
 * checked, as for gespmm_edge_segment_sum_f32; repeated entries are legal), and
 *   C[r, h F + f] = fmaf(val[order[p] H + h], B[colind[p] N + h F + f], acc)   over the entries p of row r, ascending
 * — bit for bit the unordered entry on the gathered array val_o[p, :] = val[order[p], :], without that array: the backward of an
 * attention layer is this product on the CSC arrays with order = the CSC-position -> CSR-position map. order == NULL is the unordered
 * entry, through the same code path. _x16: B and C in fp16 / bf16 as gespmm_csr_spmm_heads_x16, one rounding at the store.
 * Routes: 1 = ONE kernel exactly where gespmm_heads_route / gespmm_heads_x16_route answer 1 for the sizes and alignments (there is no
 * route query of its own): the unordered kernel with the tile staging reading order[] one tile further ahead than the weights and
 * gathering each entry's H words (16-byte loads for H = 4 / 8 on a 16-byte aligned val, 8-byte loads for H = 2 / 4 / 8 on 8 bytes,
 * dwords otherwise); allocates nothing, capturable. 0 = the composition — gespmm_edge_gather of val through order into a stream-ordered
 * temporary from the library's pool, then the unordered entry; the same bits; on a capturing stream it returns
 * hipErrorStreamCaptureUnsupported and launches nothing. GESPMM_HEADS_ORDER_ROUTE=composition pins route 0 (a measurement knob, read
 * with getenv on every call).
 * Checks: those of the unordered entries, and order not 4-byte aligned -> GESPMM_EALIGN. nnz == 0 gives C = all-zero bits and reads no
 * edge array. The plan form: a storage-order plan takes the route above; a clustered plan composes order into the permuted copy of the
 * weights it makes on every call (one pass, one buffer) and runs its task-table kernel.
 */
int gespmm_csr_spmm_heads_order_f32(const int32_t* rowptr, const int32_t* colind, const int32_t* order, const float* val, const float* B,
                                    float* C, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, void* stream);
int gespmm_csr_spmm_heads_order_x16(const int32_t* rowptr, const int32_t* colind, const int32_t* order, const float* val, const void* B,
                                    void* C, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, void* stream);
int gespmm_plan_spmm_heads_order_f32(gespmm_plan* plan, const int32_t* order, const float* val, const float* B, float* C, int64_t H,
                                     int64_t F, void* stream);
/*
 * Row gather of an edge array (since 0.5): out[i, :] = x[order[i], :] for i < n, rows of row_bytes bytes (a multiple of 4, at most 64),
 * order int32 (order_is_64 == 0) or int64 (1). One grid-stride kernel with 64-bit addressing; consecutive lanes write consecutive words
 * of out, or 16-byte pieces where row_bytes is a multiple of 16 and x and out are 16-byte aligned. Memory-safe: an index outside
 * [0, n) is never used as an address, and its row of out is written as all-ones words (NaN as fp32 / bf16 / fp16, -1 as an integer) so
 * that it shows. x and out must not overlap. n < 0, a bad row_bytes or order_is_64 -> GESPMM_EINVAL; n beyond the entry limit of the
 * products -> GESPMM_ERANGE; n == 0 -> 0 without looking at pointers; NULL -> GESPMM_EINVAL; x or out not 4-byte aligned, order not
 * aligned to its element -> GESPMM_EALIGN.
 */
int gespmm_edge_gather(const void* x, const void* order, int order_is_64, void* out, int64_t n, int64_t row_bytes, void* stream);
/*
 * Kernel choice by MEASUREMENT instead of by rule: runs the candidates of a clustered plan (batch-stream, segmented-stream,
 * staged-rows where the width is served, and at N <= 64 the batch-stream kernel with 4 floats per lane) `reps` (0 = 3) times each on these operands, synchronously, and fixes the plan
 * on the fastest; C holds the product afterwards (every candidate gives the same bits). N must be the plan's width. A no-op
 * for storage-order plans and plans created with an explicit kernel. Not under stream capture. gespmm_plan_describe reports
 * the measured times.
 */
int gespmm_plan_tune(gespmm_plan* plan, const float* B, float* C, int64_t N, int32_t reps, void* stream);
/* max reducer (unweighted plans only), see gespmm_csr_spmm_max_f32 */
int gespmm_plan_spmm_max_f32(gespmm_plan* plan, const float* B, float* C, int64_t N, float empty_value, void* stream);
/* SDDMM on the plan's pattern, out[nnz] in the caller's CSR edge order (same bits as gespmm_sddmm_csr_f32); a clustered
 * plan whose order is modelled to hit L2 walks the edges in its own order (shared rows of D2 come from L2) and scatters the
 * results back; otherwise the call is gespmm_sddmm_csr_f32 on the arrays the plan was made from (keep them alive). */
int gespmm_plan_sddmm_f32(gespmm_plan* plan, const float* D1, const float* D2, float* out, int64_t N, void* stream);
/* ... on 16-bit operands (gespmm_sddmm_csr_x16's bits): the same three routes, decided by the same rule (gespmm_plan_sddmm_route),
 * on the same row ids / edge maps / fp32 temporary the plan keeps for the fp32 call. */
int gespmm_plan_sddmm_x16(gespmm_plan* plan, const void* D1, const void* D2, float* out, int dtype, int64_t N, void* stream);
/* host only (since 0.5): which way the call above goes at width N. 0 gespmm_sddmm_csr_f32 on the caller's arrays, 1 the COO form on row
 * ids the plan expands once, 2 the plan's clustered edge order + a scatter into the caller's order. */
int gespmm_plan_sddmm_route(const gespmm_plan* plan, int64_t N);
/*
 * Multi-head SDDMM (since 0.5): the edge dot products of an attention layer, all heads in one call. D1 is [M x H F], D2 is [K x H F],
 * out is [nnz x H], fp32, contiguous, row-major:
 *
 *     out[e H + h] = dot( D1[row(e), h F : (h + 1) F], D2[col(e), h F : (h + 1) F] )
 *
 * in the summation order of gespmm_sddmm_*_f32 at WIDTH F: the (V, W) gespmm_describe_sddmm answers for N = F and the two operand
 * alignments. Head h has the bits of gespmm_sddmm_csr_f32 on contiguous copies of the two head slices with the same alignment class
 * (16-byte aligned operands: any 16-byte aligned copies). The bits depend on F and the two alignments only — not on H, the form, the
 * route, a plan or stream capture.
 * Routes: "kernel" — ONE launch, a wavefront resolves the row and column of each of its edges once for all H heads; never allocates;
 * taken wherever it can run: H >= 2 and nnz H <= 2^31 - 4097, whatever the pattern (also at mean degree >= 64, where
 * gespmm_sddmm_csr_f32 walks rows: measured faster there). "composition" — CSR calls past the pair limit: per head, the two
 * slices copied into stream-ordered temporaries of the caller's alignment class, gespmm_sddmm_csr_f32's launch at width F, a scatter into
 * out[:, h]; not on a capturing stream (hipErrorStreamCaptureUnsupported, nothing launched). The call does not carry the number of rows
 * of D2: the composition finds the largest column index on the device and WAITS for the stream once (through a plan, which knows K, it
 * does not). "plain" — H == 1: gespmm_sddmm_*_f32.
 * GESPMM_SDDMM_HEADS_ROUTE=kernel|composition pins the route (a measurement knob, read with getenv on every call and describe; "kernel"
 * is ignored where the kernel cannot run, "composition" in COO form and on a capturing stream).
 * Checks, before any device work and in the order of gespmm_sddmm_*_f32: negative sizes or H < 1 -> GESPMM_EINVAL; M, nnz, H, H F (and,
 * in COO form, nnz H) out of range -> GESPMM_ERANGE; nnz == 0 -> 0 without looking at pointers; NULL -> GESPMM_EINVAL; a pointer not
 * 4-byte aligned -> GESPMM_EALIGN. F == 0 writes nnz H zeros. fp32 operands; fp16 / bf16: the *_heads_x16 forms below.
 */
int gespmm_sddmm_coo_heads_f32(const int32_t* rowind, const int32_t* colind, const float* D1, const float* D2, float* out, int64_t H,
                               int64_t F, int64_t nnz, void* stream);
int gespmm_sddmm_csr_heads_f32(const int32_t* rowptr, const int32_t* colind, const float* D1, const float* D2, float* out, int64_t M,
                               int64_t H, int64_t F, int64_t nnz, void* stream);
/* host only: what the two calls above do, as text — "route=kernel form=csr-edge V=4 W=4 epw=16" (epw: EDGES per wavefront, 1 .. 256),
 * "route=composition V=4 W=4", "route=plain " followed by gespmm_describe_sddmm's line at width F, "route=zeros" (F == 0) or "form=none"
 * (nnz == 0). Arguments and return value as gespmm_describe_sddmm. */
int gespmm_describe_sddmm_heads(int csr, int64_t M, int64_t nnz, int64_t H, int64_t F, int d1_align, int d2_align, int capturing, char* out,
                                int64_t capacity);
/*
 * The multi-head SDDMM on 16-bit operands (since 0.5): D1 [M x H F] and D2 [K x H F] both IEEE fp16 or both bfloat16 (dtype as in
 * gespmm_sddmm_csr_x16), out fp32 [nnz x H]. Head h has the bits of gespmm_sddmm_csr_x16 on contiguous copies of the two head slices
 * with the same alignment class, at the (V, W) gespmm_describe_sddmm_x16 answers for N = F: V counts elements (up to 8), divides F, and
 * 2 V bytes divide both base addresses. Routes, pin and checks are those of the fp32 forms above — the composition copies 16-bit slices
 * and calls gespmm_sddmm_csr_x16's launch per head — with the dtype checked first (GESPMM_EINVAL) and D1 / D2 2-byte aligned.
 */
int gespmm_sddmm_coo_heads_x16(const int32_t* rowind, const int32_t* colind, const void* D1, const void* D2, float* out, int dtype,
                               int64_t H, int64_t F, int64_t nnz, void* stream);
int gespmm_sddmm_csr_heads_x16(const int32_t* rowptr, const int32_t* colind, const void* D1, const void* D2, float* out, int dtype,
                               int64_t M, int64_t H, int64_t F, int64_t nnz, void* stream);
/* host only: gespmm_describe_sddmm_heads for the two calls above (alignments from 2 bytes) */
int gespmm_describe_sddmm_heads_x16(int csr, int64_t M, int64_t nnz, int64_t H, int64_t F, int d1_align, int d2_align, int capturing,
                                    char* out, int64_t capacity);
/* ... on the plan's pattern, out in the caller's CSR edge order, the same bits. The three routes of gespmm_plan_sddmm_f32, decided by the
 * same rule at the width of the gathered row, H F (gespmm_plan_sddmm_heads_route: 0 the stateless CSR call, 1 the COO form of the heads
 * kernel on row ids the plan expands once, 2 the clustered edge order into a plan-owned [nnz, H] temporary + a scatter of H words per
 * edge; 0 as well where nnz H is past the kernel's limit). The route-2 temporary is made by the first call that needs it and again when
 * H grows — never on a capturing stream (hipErrorStreamCaptureUnsupported, nothing launched) — and freed with the plan. */
int gespmm_plan_sddmm_heads_f32(gespmm_plan* plan, const float* D1, const float* D2, float* out, int64_t H, int64_t F, void* stream);
int gespmm_plan_sddmm_heads_route(const gespmm_plan* plan, int64_t H, int64_t F);
/*
 * Edge softmax over the entries of each CSR row, per head (since 0.5): the step between the scores of an attention layer
 * (gespmm_sddmm_csr_heads_f32) and its aggregation (gespmm_csr_spmm_heads_f32). score and out are [nnz x H], fp32, contiguous,
 * row-major, in CSR edge order; rowptr has M + 1 entries and rowptr[M] == nnz. For row r with entries [lo, hi) and head h:
 *
 *     x_p = score[p H + h] >= 0 ? score[p H + h] : slope * score[p H + h]        (leaky ReLU; slope == 1: none, no multiply)
 *     out[p H + h] = exp(x_p - max_p x_p) / sum_p exp(x_p - max_p x_p)
 *
 * Empty rows write nothing. A NaN or +inf score, or a row of -inf only, makes its own (row, head) NaN and nothing else; -inf among
 * finite scores gives +0. The exponential is exp2(fl(x log2(e))) on the hardware's exp2 (results below 2^-126 flush to zero).
 * Summation order (pinned): a row of d <= L entries is folded by W lanes — lane l takes entries lo + l + t W in order, fmaxf for the
 * maximum, plain adds for the sum, then an xor butterfly with masks W/2 .. 1 — and a row of d > L entries the same way by 64 lanes.
 * W is the smallest power of two >= ceil(nnz / M) within [4, 16], L = 2048 (gespmm_describe_edge_softmax prints both). Head h of a call
 * has the bits of the H = 1 call on a contiguous copy of score[:, h]; the bits do not depend on H, on stream capture or on the run.
 * One kernel, no atomics, no workspace, no allocation, no host synchronisation: it can be captured in a graph.
 * Checks, before any device work and in this order: H < 1, a negative size, M == 0 with nnz > 0, a NaN or infinite slope ->
 * GESPMM_EINVAL; M > 2^31 - 4097, or nnz H > 2^31 - 4097 (32-bit word positions; there is no other route) -> GESPMM_ERANGE; nnz == 0 -> 0
 * without looking at pointers; NULL -> GESPMM_EINVAL; a pointer not 4-byte aligned -> GESPMM_EALIGN. out must not overlap score or rowptr
 * (not checked). fp32 only.
 */
int gespmm_edge_softmax_f32(const int32_t* rowptr, const float* score, float* out, int64_t M, int64_t H, int64_t nnz, float slope,
                            void* stream);
/*
 * Its backward (since 0.5): alpha is the forward's output, grad_alpha the gradient with respect to it, both [nnz x H];
 *
 *     dot = sum_p alpha_p grad_alpha_p                  (fmaf chains in the forward's lane order, then the butterfly)
 *     grad_score[p H + h] = alpha_p * (grad_alpha_p - dot) * (score_p >= 0 ? 1 : slope)
 *
 * score (the forward's input) is read for its sign only, and only when slope != 1: it must be NULL or is ignored when slope == 1. Same
 * checks, order and limits as the forward; grad_score must not overlap an input (not checked).
 */
int gespmm_edge_softmax_backward_f32(const int32_t* rowptr, const float* alpha, const float* grad_alpha, const float* score,
                                     float* grad_score, int64_t M, int64_t H, int64_t nnz, float slope, void* stream);
/* host only (since 0.5): the launch shape of the two calls above, from the function the launch itself runs — "W=8 long_rows>2048" (lanes
 * per (row, head) pair; rows of more entries than that take a whole wavefront) or "form=none" (nnz == 0). H never changes the answer.
 * out / capacity / return value as gespmm_describe_sddmm: the text is truncated to capacity - 1 characters and NUL-terminated, the
 * return value is the number of characters written, or a GESPMM_E* code for sizes the calls above refuse. */
int gespmm_describe_edge_softmax(int64_t M, int64_t nnz, int64_t H, char* out, int64_t capacity);
/*
 * The edge softmax on the additive score of a graph attention layer (since 0.5), with no score array:
 *
 *     score[p, h] = fl(el[r H + h] + er[colind[p] H + h])        (one fp32 add; r = the row of entry p)
 *     out = gespmm_edge_softmax_f32(rowptr, score, ..)           bit for bit, in ONE kernel that writes out only
 *
 * el is [M x H], er [K x H], out [nnz x H], fp32, contiguous, row-major; colind has nnz entries within [0, K) (a precondition, not
 * checked). These are the bits of gespmm_sddmm_csr_heads_f32 at F = 2 on q = (el, 1), k = (1, er) followed by the softmax above: the
 * width-2 chain fmaf(1, er, fmaf(el, 1, 0)) is fl(el + er). Lane geometry, W, L and the summation order are the softmax's own
 * (gespmm_describe_edge_softmax(M, nnz, H)); a row of more than 4 W entries gathers colind and er again in each of its three sweeps.
 * A NaN or +inf in el makes the (row, head) pairs of its own row NaN and nothing else.
 * Checks, in this order: what gespmm_edge_softmax_f32 answers GESPMM_EINVAL for on (M, H, nnz, slope), or K < 1 -> GESPMM_EINVAL; its
 * range limits, or M H or K H > 2^31 - 4097 (32-bit word positions) -> GESPMM_ERANGE; nnz == 0 -> 0 without looking at pointers; NULL -> GESPMM_EINVAL; a pointer not 4-byte
 * aligned -> GESPMM_EALIGN. out must not overlap an input (not checked). No atomics, no workspace, no allocation: capturable.
 */
int gespmm_gat_softmax_f32(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, float* out, int64_t M, int64_t K,
                           int64_t H, int64_t nnz, float slope, void* stream);
/*
 * Its backward (since 0.5), one kernel: grad_score [nnz x H] has the bits of gespmm_edge_softmax_backward_f32 with score = fl(el + er)
 * (colind, el, er are read for that sign only, and only when slope != 1: they may be NULL when slope == 1), and
 *
 *     grad_el[r H + h] = sum over the entries p of row r of grad_score[p H + h]          (the fp32 values as stored)
 *
 * [M x H], every word written (an empty row: +0). Summation order (pinned): lane l of the row's W lanes adds its entries lo + l + t W
 * in entry order with plain adds starting from +0, then the xor butterfly with masks W/2 .. 1; rows of more than L entries the same at
 * W = 64. grad_er is gespmm_edge_segment_sum_f32 of grad_score on the CSC arrays. Checks as the forward; nnz == 0 looks at grad_el
 * alone (NULL -> GESPMM_EINVAL, alignment) and zero-fills it.
 */
int gespmm_gat_softmax_backward_f32(const int32_t* rowptr, const int32_t* colind, const float* alpha, const float* grad_alpha,
                                    const float* el, const float* er, float* grad_score, float* grad_el, int64_t M, int64_t K, int64_t H,
                                    int64_t nnz, float slope, void* stream);
/*
 * Per-segment sum of an edge array (since 0.5): out[s H + h] = sum over p in [ptr[s], ptr[s + 1]) of x[(order ? order[p] : p) H + h].
 * ptr has S + 1 entries, ptr[S] == nnz; x is [nnz x H]; order is NULL or a permutation-like int32[nnz] within [0, nnz) (not checked);
 * out is [S x H], every word written (an empty segment: +0). The geometry and the pinned order above, with W and L from
 * gespmm_describe_edge_softmax(S, nnz, H); on (rowptr, NULL) it reproduces grad_el of the call above bit for bit, on (colptr,
 * csc_order) it gives grad_er with no permuted copy of grad_score. Checks: H < 1, a negative size, S == 0 with nnz > 0 ->
 * GESPMM_EINVAL; S > 2^31 - 4097, nnz H or S H > 2^31 - 4097 -> GESPMM_ERANGE; S == 0 -> 0; nnz == 0 looks at out alone and
 * zero-fills it; NULL (ptr, x, out) -> GESPMM_EINVAL; alignment -> GESPMM_EALIGN. One kernel, capturable.
 */
int gespmm_edge_segment_sum_f32(const int32_t* ptr, const int32_t* order, const float* x, float* out, int64_t S, int64_t H, int64_t nnz,
                                void* stream);
/*
 * The row statistics of gespmm_gat_softmax_f32 (since 0.5): stats is [M x H x 2], fp32, 8-byte aligned, and for row r, head h, with
 * x(r, c, h) = leaky(fl(el[r H + h] + er[c H + h]), slope)
 *
 *     stats[r, h, 0] = m = the maximum of x over the row's entries,    stats[r, h, 1] = s = the sum of __expf(x - m) over them
 *
 * with EXACTLY the bits gespmm_gat_softmax_f32 uses for that pair: the same kernel — lane geometry W / L of
 * gespmm_describe_edge_softmax(M, nnz, H), the register and the sweep regime, the fmaxf chain and xor butterfly, the `s += t` chain in
 * which a masked lane adds +0, the W = 64 branch for rows of more than L entries — without its last pass; one 8-byte store per pair.
 * Every word is written; an empty row writes (+0, +0). Checks: the ladder of gespmm_gat_softmax_f32; M == 0 -> 0; nnz == 0 looks at
 * stats alone and zero-fills it (hipMemsetAsync); stats not 8-byte aligned -> GESPMM_EALIGN. One kernel, no workspace: capturable.
 */
int gespmm_gat_softmax_stats_f32(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, float* stats, int64_t M,
                                 int64_t K, int64_t H, int64_t nnz, float slope, void* stream);
/*
 * The aggregation of a graph attention layer with no attention array (since 0.5). el [M x H], er [K x H], stats [M x H x 2] (the call
 * above) are the same arrays in both modes; the weight of row index r, column index c, head h is
 *
 *     w(r, c, h) = __expf(x(r, c, h) - stats[r, h, 0]) / stats[r, h, 1]        (the bits of gespmm_gat_softmax_f32's out)
 *
 *     transposed == 0   (ptr, ind) = (rowptr[M + 1], colind)   B [K x H F]   C [M x H F]   entry p of segment i, j = ind[p]: w(i, j, h)
 *     transposed == 1   (ptr, ind) = (colptr[K + 1], rowind)   B [M x H F]   C [K x H F]   entry p of segment i, j = ind[p]: w(j, i, h)
 *
 *     C[i, h F + f] = fmaf(w, B[j, h F + f], acc) over the segment's entries, ascending, from +0
 *
 * — one fp32 chain per output element in strict order. transposed == 0 has the bits of gespmm_csr_spmm_heads_f32(rowptr, colind,
 * alpha, B) with alpha = gespmm_gat_softmax_f32(..); transposed == 1 those of gespmm_csr_spmm_heads_f32(colptr, rowind, alpha in CSC
 * order, B): the product of the backward, without alpha and without its permuted copy. A NaN or inf in el poisons what it poisons
 * there. nnz == 0 gives C = 0 (hipMemsetAsync).
 * Routes (gespmm_gat_aggregate_route): 1 = ONE kernel — the multi-head batch-stream kernel computing its staged weights — for
 * 1 <= H <= 8, 32-bit offsets (rows of B x H F x 4 < 2^32, nnz H < 2^31) and the lane geometries gespmm_heads_route serves; no
 * workspace, no allocation: capturable. 0 = the composition: the weights into a stream-ordered temporary [nnz x H] from the library's
 * pool (the same expression: the same bits), then gespmm_csr_spmm_heads_f32; on a capturing stream it returns
 * hipErrorStreamCaptureUnsupported and launches nothing. GESPMM_GAT_AGGREGATE_ROUTE=composition pins route 0 (a measurement knob,
 * read with getenv on every call).
 * Checks, in this order: transposed not 0 / 1, F < 0, then the ladder of gespmm_gat_softmax_f32 on (M, K, H, nnz, slope), then that of
 * gespmm_csr_spmm_heads_f32 on the width; no segments (M == 0, transposed == 0) or F == 0 -> 0; nnz == 0 looks at C alone; NULL ->
 * GESPMM_EINVAL; a pointer not 4-byte (stats: 8-byte) aligned -> GESPMM_EALIGN. C must not overlap an input (not checked).
 */
int gespmm_gat_aggregate_f32(const int32_t* ptr, const int32_t* ind, const float* el, const float* er, const float* stats, const float* B,
                             float* C, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, int transposed, void* stream);
/* Host only: the route of the call above for these sizes and operand alignments, as gespmm_heads_route — 1 or 0, or a GESPMM_E*
 * code; geometry_out (may be NULL): V, strips, W, rows per wavefront of route 1, zeros for route 0. */
int gespmm_gat_aggregate_route(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, int transposed, int b_align, int c_align,
                               int32_t* geometry_out);
/*
 * The backward of a graph attention layer for its two score terms with no [nnz x H] array (since 0.5). el [M x H], er [K x H], stats
 * [M x H x 2] as above; grad_out [M x H x F] is the gradient of gespmm_gat_aggregate_f32's C, feat [K x H x F] its B. For entry p of
 * row r, column c, head h
 *
 *     g_p = sum_f grad_out[r, h, f] feat[c, h, f]             delta[r, h] = sum over row r of w(r, c, h) g_p
 *     gs_p = w(r, c, h) (g_p - delta[r, h]) (fl(el[r H + h] + er[c H + h]) >= 0 ? 1 : slope)         (the factor only when slope != 1)
 *     grad_el[r, h] = sum over row r of gs_p                  grad_er[c, h] = sum over column c of gs_p
 *
 * gespmm_gat_backward_el_f32 walks the rows (rowptr, colind) and writes delta and grad_el [M x H]; gespmm_gat_backward_er_f32 walks
 * the columns (colptr, rowind: the CSC arrays, no csc_order), reads delta and writes grad_er [K x H]. gs_p is computed in both, from
 * node-sized words alone, with the same bits. Lane geometry: the edge softmax's, W and L from gespmm_describe_edge_softmax(M, nnz, H)
 * for the rows and (K, nnz, H) for the columns. Pinned orders: g_p is ONE fmaf chain over ascending f from +0, whatever F, the
 * alignment (16-byte loads when F % 4 == 0 and grad_out and feat are 16-byte aligned, 4-byte loads otherwise) or the mode; delta is
 * the dot of gespmm_gat_softmax_backward_f32 (fmaf(w, g, dot) per lane in entry order, then the xor butterfly W/2 .. 1); gs_p is
 * `r = w * (g - delta); r *= factor`; grad_el and grad_er are the chain of gespmm_edge_segment_sum_f32 (plain adds from +0, then the
 * butterfly). Where g_p has the bits gespmm_sddmm_csr_heads_f32 gives it (always when its partial sums are exact), delta, grad_el and
 * grad_er have the bits of gespmm_gat_softmax_f32 + gespmm_sddmm_csr_heads_f32 + gespmm_gat_softmax_backward_f32 +
 * gespmm_edge_segment_sum_f32(colptr, .., csc_order). Every word of the results is written (an empty row or column: +0).
 * Checks, in this order: the ladder of gespmm_gat_aggregate_f32 on (M, K, H, F, nnz, slope) in both directions; M H F or K H F >
 * 2^31 - 4097 -> GESPMM_ERANGE; gespmm_gat_backward_el_f32 with M == 0 -> 0; nnz == 0 or F == 0 looks at the results alone and
 * zero-fills them (hipMemsetAsync); NULL -> GESPMM_EINVAL; a pointer not 4-byte (stats: 8-byte) aligned -> GESPMM_EALIGN. One kernel
 * each, no atomics, no workspace, no allocation: capturable. The results must not overlap an input (not checked).
 */
int gespmm_gat_backward_el_f32(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, const float* stats,
                               const float* grad_out, const float* feat, float* delta, float* grad_el, int64_t M, int64_t K, int64_t H,
                               int64_t F, int64_t nnz, float slope, void* stream);
int gespmm_gat_backward_er_f32(const int32_t* colptr, const int32_t* rowind, const float* el, const float* er, const float* stats,
                               const float* delta, const float* grad_out, const float* feat, float* grad_er, int64_t M, int64_t K, int64_t H,
                               int64_t F, int64_t nnz, float slope, void* stream);
/*
 * Dropout on the attention coefficients with a mask that is never stored (new symbols of 0.5). Whether entry (r, c) of the pattern
 * keeps head h is a pure function of (seed, r, c, h), in uint32 arithmetic:
 *
 *     mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
 *     bits(s0, s1, r, c, h) = mix( mix( mix(r ^ s0) ^ c ) ^ (h * 0x9E3779B9) ^ s1 )
 *     keep = bits >= T,  T = min(floor((double)p 2^32), 2^32 - 1)         dropout(x) = keep ? x * s : +0,  s = 1.0f / (1.0f - p)
 *
 * dropout is a select: a dropped NaN or inf becomes +0. r and c are the row and the column of the entry whichever way the pattern is
 * walked, so the walk over rows (rowptr, colind) and the walk over columns (colptr, rowind; no CSR position, no csc_order) recompute
 * the same decision. Two entries with the same (r, c) — a multigraph — therefore share theirs. `seed` is a DEVICE pointer to two
 * 32-bit words, 4-byte aligned, read by the kernels with ordinary loads and never written: no host synchronisation, and a seed drawn
 * or overwritten on the device between two replays of a captured graph changes the mask. p == 0 is legal (T = 0, s = 1: the bits of
 * the base entry point).
 * Known answers with (s0, s1) = (0x12345678, 0x9abcdef0): bits(0, 0, 0) = 0xffb6cd07, bits(1, 5, 1) = 0xf2651a06,
 * bits(2, 2, 7) = 0x8cee38f8, bits(511, 300, 3) = 0x75f57072.
 *
 * gespmm_edge_dropout_f32: y[p H + h] = dropout(x[p H + h]) for entry p of the CSR pattern, [nnz x H]; y == x is allowed. Forward on
 * alpha and backward on its gradient: the op is its own adjoint. One grid-stride kernel, no workspace: capturable. Checks: the ladder
 * of gespmm_gat_softmax_f32 on (M, K, H, nnz), !(0 <= p < 1) (NaN included) -> GESPMM_EINVAL with the other senseless arguments;
 * nnz == 0 -> 0; NULL (seed included) -> GESPMM_EINVAL; not 4-byte aligned -> GESPMM_EALIGN.
 *
 * gespmm_gat_aggregate_dropout_f32: gespmm_gat_aggregate_f32 with the staged weight dropout(w(r, c, h)) — the bits of
 * gespmm_csr_spmm_heads_f32 on gespmm_edge_dropout_f32(gespmm_gat_softmax_f32(..)), for transposed == 1 on the CSC arrays with that
 * array permuted. Route 0 applies the same expression to its temporary. stats are those of the softmax WITHOUT dropout: it comes after
 * the normalisation.
 *
 * gespmm_gat_backward_el_dropout_f32 / _er_dropout_f32: the fused backward with g_p replaced by g'_p = dropout(g_p) directly after its
 * chain (one rounding fl(g_p s), or +0); delta = sum w g', gs_p = w (g'_p - delta) factor with w the UNDROPPED weight. Where the dot's
 * partial sums are exact, the bits of gespmm_gat_softmax_f32 + gespmm_sddmm_csr_heads_f32 + gespmm_edge_dropout_f32 +
 * gespmm_gat_softmax_backward_f32 + gespmm_edge_segment_sum_f32.
 *
 * The three fused forms follow their base entry's ladder: a bad p joins the step that rejects a bad slope, a NULL seed the NULL step,
 * a misaligned seed the alignment step; nnz == 0 behaves as in the base entry (the seed is still checked).
 */
int gespmm_edge_dropout_f32(const int32_t* rowptr, const int32_t* colind, const float* x, float* y, int64_t M, int64_t K, int64_t H,
                            int64_t nnz, float p, const void* seed, void* stream);
int gespmm_gat_aggregate_dropout_f32(const int32_t* ptr, const int32_t* ind, const float* el, const float* er, const float* stats,
                                     const float* B, float* C, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope,
                                     int transposed, float p, const void* seed, void* stream);
int gespmm_gat_backward_el_dropout_f32(const int32_t* rowptr, const int32_t* colind, const float* el, const float* er, const float* stats,
                                       const float* grad_out, const float* feat, float* delta, float* grad_el, int64_t M, int64_t K,
                                       int64_t H, int64_t F, int64_t nnz, float slope, float p, const void* seed, void* stream);
int gespmm_gat_backward_er_dropout_f32(const int32_t* colptr, const int32_t* rowind, const float* el, const float* er, const float* stats,
                                       const float* delta, const float* grad_out, const float* feat, float* grad_er, int64_t M, int64_t K,
                                       int64_t H, int64_t F, int64_t nnz, float slope, float p, const void* seed, void* stream);
/* Host only: the mask's bits and the threshold T as the kernels compute them. gespmm_edge_dropout_threshold answers 0xffffffff for a p
 * outside [0, 1), which no legal p gives. */
uint32_t gespmm_edge_dropout_bits(uint32_t s0, uint32_t s1, uint32_t r, uint32_t c, uint32_t h);
uint32_t gespmm_edge_dropout_threshold(float p);
/*
 * The GATv2 edge score (Brody et al.) and its gradients with nothing larger than [nnz x H] (new symbols of 0.5). xl [M x H x F] is the
 * aggregating node's term (the row of an entry), xr [K x H x F] the neighbour's (the column), att [H x F]; score is [nnz x H] in CSR
 * entry order, head-minor — what gespmm_edge_softmax_f32 reads:
 *
 *     score[p H + h] = sum_f att[h, f] leaky(fl(xl[row(p), h, f] + xr[col(p), h, f]))      leaky(t) = t >= 0 ? t : slope t
 *
 * (one fp32 add; slope == 1: no multiply). One kernel in the geometry of gespmm_sddmm_csr_heads_f32, att's head slice a third operand:
 * (V, W, epw) from gespmm_describe_gatv2_score for width F and the THREE operand addresses (V divides F, 4 V bytes divide all three).
 * Pinned order: lane l of W runs ONE chain acc = fmaf(att[h, j], leaky(fl(xl_j + xr_j)), acc) from +0 over j = l V + i + t W V (i
 * ascending inside a vector, t ascending), then the xor butterfly W/2 .. 1; a lane past the slice contributes fmaf(0, 0, 0).
 *
 * gespmm_gatv2_score_backward_f32 serves both node terms. For segment s with entries p in [ptr[s], ptr[s + 1]), c = ind[p],
 * q = order ? order[p] : p and t = fl(x_seg[s, h, f] + x_ind[c, h, f]):
 *
 *     m_pf              = t >= 0 ? att[h, f] : fl(att[h, f] slope)                (att[h, f] for every t when slope == 1)
 *     grad_x[s, h, f]   = chain over p ascending from +0 of fmaf(grad_score[q H + h], m_pf, acc)
 *     att_part[s, h, f] = chain over p ascending from +0 of fmaf(grad_score[q H + h], leaky(t), acc)       (only when att_part != NULL)
 *
 * Row pass (grad_xl and att_part): ptr = rowptr, ind = colind, order = NULL, x_seg = xl, x_ind = xr, S = M, T = K. Column pass
 * (grad_xr): ptr = colptr, ind = rowind, order = csc_order, x_seg = xr, x_ind = xl, att_part = NULL, S = K, T = M. fp32 addition
 * commutes bit for bit: both passes see the same t. The gradient of att is att_part summed over s by the caller. Pinned order: ONE
 * fp32 fmaf chain per output word in segment order (the contract of gespmm_csr_spmm_heads_f32); lane geometry and vector width (16-byte
 * loads when F % 4 == 0 and x_seg, x_ind, att and the results are 16-byte aligned, 4-byte loads otherwise) leave no trace in the bits.
 * There is no long-row pass: a hub segment is walked by one lane group. Every word of grad_x (and att_part) is written, +0 for an
 * empty segment.
 * Checks, in this order (S, T stand for M, K in the forward): a negative size, H < 1, T < 1 or S < 1 with nnz > 0, a NaN or infinite
 * slope -> GESPMM_EINVAL; S, nnz, nnz H, S H F or T H F > 2^31 - 4097 -> GESPMM_ERANGE (32-bit word positions, no other route);
 * forward: nnz == 0 -> 0 without looking at pointers; backward: nnz == 0 or F == 0 looks at the results alone and zero-fills them;
 * forward: F == 0 zero-fills score; NULL (order and att_part may be NULL) -> GESPMM_EINVAL; a pointer not 4-byte aligned ->
 * GESPMM_EALIGN. No atomics, no workspace, no allocation, no host synchronisation: capturable. Results must not overlap an input.
 */
int gespmm_gatv2_score_f32(const int32_t* rowptr, const int32_t* colind, const float* xl, const float* xr, const float* att, float* score,
                           int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, void* stream);
int gespmm_gatv2_score_backward_f32(const int32_t* ptr, const int32_t* ind, const int32_t* order, const float* grad_score,
                                    const float* x_seg, const float* x_ind, const float* att, float* grad_x, float* att_part, int64_t S,
                                    int64_t T, int64_t H, int64_t F, int64_t nnz, float slope, void* stream);
/* Host only: what gespmm_gatv2_score_f32 would launch, as text: "V=.. W=.. epw=..", "route=zeros" (F == 0) or "form=none" (nnz == 0).
 * *_align: largest power of two (>= 4) dividing the operand's address. Returns the length written or a GESPMM_E* code. */
int gespmm_describe_gatv2_score(int64_t M, int64_t nnz, int64_t H, int64_t F, int xl_align, int xr_align, int att_align, char* out,
                                int64_t capacity);
/*
 * The GATv2 edge score and its gradients on 16-bit node operands (new symbols of 0.5). xl, xr, x_seg, x_ind and grad_x are IEEE fp16 or
 * bfloat16 (dtype: GESPMM_X16_F16 / GESPMM_X16_BF16, one type per call); att, grad_score, score and att_part stay fp32 — att is a
 * parameter of H F words whose gradient is a sum over nodes, and everything edge-sized is fp32 in this library. The arithmetic is that
 * of the fp32 pair above, unchanged: every 16-bit element is widened exactly at its use (subnormals included),
 *
 *     t = fl32(widen(xl[row(p), h, f]) + widen(xr[col(p), h, f]))                      ONE fp32 add; the leaky branch is t >= 0
 *
 * the forward is the pinned lane chain acc = fmaf(att_j, leaky(t_j), acc) over j = l V + i + t W V and the xor butterfly (a lane past
 * the slice contributes fmaf(0, 0, 0)), the backward ONE fp32 fmaf chain per output word in segment order with m = t >= 0 ? att :
 * fl(att slope). grad_x is rounded ONCE, at the store: to nearest even, overflow to +-inf, NaN stays NaN. No packed-fp16 arithmetic, no
 * dot2. So att_part has the bits of gespmm_gatv2_score_backward_f32 on the widened operands, grad_x is that call's grad_x rounded once,
 * and score has the bits of gespmm_gatv2_score_f32 on the widened operands wherever the two describe calls answer the same (V, W).
 * Forward geometry (gespmm_describe_gatv2_score_x16): V counts ELEMENTS — 8 / 4 / 2 / 1, a 16 / 8 / 4 / 2-byte load of xl and xr, with
 * att's V floats at the same positions in loads of at most 16 bytes — and is the largest value that divides F, whose 2 V bytes divide
 * the addresses of xl and xr and whose min(4 V, 16) bytes divide the address of att; W and epw follow the rule of
 * gespmm_describe_sddmm_heads_x16 at width F. The bits depend on (V, W) alone. Backward geometry: the row walk at width H F with V
 * elements per lane under the same rule on x_seg, x_ind, grad_x (2 V bytes) and att, att_part (min(4 V, 16) bytes) — 16-byte vectors
 * when F % 8 == 0 and every dense operand is 16-byte aligned, V = 1 for any F and any 2-byte aligned address; no vector spans two
 * heads; geometry leaves no trace in the bits. There is no long-row pass.
 * Checks, in this order: a dtype that is neither code -> GESPMM_EINVAL; then the ladder of the fp32 pair — sizes that make no sense
 * (and a NaN or infinite slope) -> GESPMM_EINVAL; S, nnz, nnz H, S H F or T H F > 2^31 - 4097 -> GESPMM_ERANGE (32-bit ELEMENT
 * positions); forward: nnz == 0 -> 0 without looking at pointers, F == 0 zero-fills score; backward: nnz == 0 or F == 0 looks at the
 * results alone and zero-fills them; NULL (order and att_part may be NULL) -> GESPMM_EINVAL; a 16-bit operand not 2-byte aligned, or
 * any other pointer not 4-byte aligned -> GESPMM_EALIGN. No atomics, no workspace, no allocation, no host synchronisation: capturable.
 * Results must not overlap an input.
 */
int gespmm_gatv2_score_x16(const int32_t* rowptr, const int32_t* colind, const void* xl, const void* xr, const float* att, float* score,
                           int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, void* stream);
int gespmm_gatv2_score_backward_x16(const int32_t* ptr, const int32_t* ind, const int32_t* order, const float* grad_score,
                                    const void* x_seg, const void* x_ind, const float* att, void* grad_x, float* att_part, int dtype,
                                    int64_t S, int64_t T, int64_t H, int64_t F, int64_t nnz, float slope, void* stream);
/* Host only: what gespmm_gatv2_score_x16 would launch, in the words of gespmm_describe_gatv2_score. xl_align, xr_align: largest power
 * of two (>= 2) dividing the operand's address; att_align: >= 4. Returns the length written or a GESPMM_E* code. */
int gespmm_describe_gatv2_score_x16(int64_t M, int64_t nnz, int64_t H, int64_t F, int xl_align, int xr_align, int att_align, char* out,
                                    int64_t capacity);
/*
 * Fused scaled dot-product attention over the entries of a pattern (the attention of a graph transformer: PyG's TransformerConv, UniMP)
 * and its backward, with NOTHING of size nnz but the index arrays (new symbols of 0.5). q [M x H x F] is the aggregating node's term
 * (the row of an entry), k and v [K x H x F] the neighbour's (the column); out and grad_out [M x H x F], stats [M x H x 2], delta
 * [M x H]. For entry p of row r with column c and head h
 *
 *     s_p = fl(scale dot(q[r, h, :], k[c, h, :]))      a_p = exp(s_p - m) / l,  (m, l) = stats[r, h] = (max_p s_p, sum_p exp(s_p - m))
 *     out[r, h, :] = sum_p a_p v[c, h, :]
 *
 * Geometry of all three kernels: a group of W lanes owns a (segment, head) pair — rows in the forward and in _backward_q, columns in
 * _backward_kv — with V floats per load and 8 floats per lane and operand; (V, W) from gespmm_describe_dot_attention: V the widest of
 * 4 / 2 / 1 that divides F and whose bytes divide every dense operand's address, W the smallest power of two in 4 .. 64 with 8 W >= F.
 * F > 512 is not served: GESPMM_ERR_UNSUPPORTED, nothing launched. A hub segment is walked by its one lane group (a limit).
 * Pinned orders: dot(x, y): lane l runs ONE chain acc = fmaf(x_j, y_j, acc) from +0 over j = l V + i + t W V (i ascending inside a
 * vector, t ascending), then the xor butterfly W/2 .. 1; a lane past the slice contributes fmaf(0, 0, acc). fmaf commutes in its
 * factors: the row pass and the column pass of the backward see the same bits of s_p and g_p. Every per-word accumulation is one chain
 * per output word in segment (entry) order; the head, H, alignment, capture and run leave no trace beyond V.
 *
 * Forward — one sweep with an online softmax; per entry, in entry order:
 *     m' = fmaxf(m, s_p);  c = __expf(m - m');  t = __expf(s_p - m');  l = fmaf(l, c, t);  acc_f = fmaf(t, v_f, fl(acc_f c));  m = m'
 * from (m, l, acc) = (s_0, 0, 0) — the first entry gives l = 1, acc = v with no exp(-inf - ..) — and out = acc / l. Every word of out
 * and stats is written; an empty row writes +0 everywhere.
 * gespmm_dot_attention_backward_q_f32 (rowptr, colind) writes delta and grad_q:
 *     delta[r, h] = dot(grad_out[r, h, :], out[r, h, :])     g_p = dot(grad_out[r, h, :], v[c, h, :])      ds_p = a_p (g_p - delta[r, h])
 *     grad_q[r, h, f] = fl(scale chain over p of fmaf(ds_p, k[c, h, f], acc))                 with a_p = __expf(s_p - m) / l
 * gespmm_dot_attention_backward_kv_f32 (colptr, rowind: the CSC arrays, no csc_order) reads delta and writes
 *     grad_k[c, h, f] = fl(scale chain over p of fmaf(ds_p, q[r, h, f], acc))       grad_v[c, h, f] = chain of fmaf(a_p, grad_out[r, h, f], acc)
 * The *_dropout_f32 forms put dropout on a_p (the mask of gespmm_edge_dropout_f32: a function of (seed, r, c, h)): the forward's l sums
 * every entry and acc takes fl(t s) for a kept entry, +0 for a dropped one; the backward replaces g_p by fl(g_p s) or +0 directly after
 * its chain, delta stays dot(grad_out, out), grad_v uses fl(a_p s) or +0.
 * Checks, in this order: a negative size, H < 1, M < 1 or K < 1 with nnz > 0, a NaN or infinite scale, !(0 <= p < 1) -> GESPMM_EINVAL;
 * M, K, nnz, nnz H, M H F, K H F or 2 M H > 2^31 - 4097 -> GESPMM_ERANGE; F > 512 -> GESPMM_ERR_UNSUPPORTED; nnz == 0 or F == 0 looks at
 * the results (and the seed) alone and zero-fills them (hipMemsetAsync); NULL -> GESPMM_EINVAL; a pointer not 4-byte (stats: 8-byte)
 * aligned -> GESPMM_EALIGN. No atomics, no workspace, no allocation, no host synchronisation: capturable. Results must not overlap an
 * input (not checked). colind within [0, K), rowind within [0, M) and ptr[last] == nnz are preconditions.
 */
int gespmm_dot_attention_f32(const int32_t* rowptr, const int32_t* colind, const float* q, const float* k, const float* v, float* out,
                             float* stats, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, void* stream);
int gespmm_dot_attention_dropout_f32(const int32_t* rowptr, const int32_t* colind, const float* q, const float* k, const float* v, float* out,
                                     float* stats, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, float p,
                                     const void* seed, void* stream);
int gespmm_dot_attention_backward_q_f32(const int32_t* rowptr, const int32_t* colind, const float* q, const float* k, const float* v,
                                        const float* stats, const float* out, const float* grad_out, float* delta, float* grad_q, int64_t M,
                                        int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, void* stream);
int gespmm_dot_attention_backward_q_dropout_f32(const int32_t* rowptr, const int32_t* colind, const float* q, const float* k, const float* v,
                                                const float* stats, const float* out, const float* grad_out, float* delta, float* grad_q,
                                                int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, float p, const void* seed,
                                                void* stream);
int gespmm_dot_attention_backward_kv_f32(const int32_t* colptr, const int32_t* rowind, const float* q, const float* k, const float* v,
                                         const float* stats, const float* delta, const float* grad_out, float* grad_k, float* grad_v,
                                         int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, void* stream);
int gespmm_dot_attention_backward_kv_dropout_f32(const int32_t* colptr, const int32_t* rowind, const float* q, const float* k, const float* v,
                                                 const float* stats, const float* delta, const float* grad_out, float* grad_k, float* grad_v,
                                                 int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, float p,
                                                 const void* seed, void* stream);
/* Host only: what the three entry points would launch, as text: "V=.. W=..", "route=unsupported" (F > 512), "route=zeros" (F == 0) or
 * "form=none" (nnz == 0). *_align: largest power of two (>= 4) dividing the operand's address; the least of them decides V. Returns the
 * length written or a GESPMM_E* code. */
int gespmm_describe_dot_attention(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, int q_align, int k_align, int v_align, char* out,
                                  int64_t capacity);
/*
 * ... on 16-bit node terms (new symbols of 0.5): q, out, grad_out, grad_q [M x H x F] and k, v, grad_k, grad_v [K x H x F] are IEEE
 * fp16 or bfloat16 (dtype: GESPMM_X16_F16 / GESPMM_X16_BF16, one type per call); stats, delta and scale stay fp32.
 * The arithmetic is the fp32 contract above, expression for expression: every 16-bit element is widened exactly at its use (subnormals
 * included); the pinned lane dot, the xor butterfly, s_p = fl(scale dot), the online softmax, out = acc / l, a_p, g_p, ds_p, the
 * per-word chains in entry order and the dropout placement are the fp32 kernels'; every accumulation is fp32. _backward_q reads the
 * STORED, 16-bit out for delta = dot(grad_out, out). Every 16-bit result is rounded ONCE, at its store (to nearest even, overflow to
 * +-inf, NaN stays NaN); for grad_q and grad_k that is fl32(scale chain), then one rounding. No packed-fp16 arithmetic and no dot2.
 * Geometry (gespmm_describe_dot_attention_x16): the fp32 kernel's with V counted in ELEMENTS — V in {4, 2, 1}, an 8 / 4 / 2-byte load;
 * 8 elements per lane and operand; W the smallest power of two in 4 .. 64 with 8 W >= F; V the widest of 4 / 2 / 1 that divides F and
 * whose 2 V bytes divide the address of every 16-bit operand and result of the launch. A 16-byte load form (V = 8) is deliberately not
 * built. Lane positions, chains and orders are those of the fp32 kernels at the same (V, W): wherever gespmm_describe_dot_attention
 * answers the same (V, W) for the widened operands (a 16-bit operand b bytes off a 16-byte boundary corresponds to an fp32 operand 2 b
 * bytes off), stats and delta have the BITS of the fp32 entry points on the widened operands — _backward_q fed widen(out),
 * _backward_kv fed that delta — and out, grad_q, grad_k and grad_v are those calls' results narrowed once.
 * Checks, in this order: a dtype that is neither code -> GESPMM_EINVAL; then the fp32 ladder with limits in ELEMENT positions (sizes
 * that make no sense -> GESPMM_EINVAL; M, K, nnz, nnz H, M H F, K H F or 2 M H > 2^31 - 4097 -> GESPMM_ERANGE; F > 512 ->
 * GESPMM_ERR_UNSUPPORTED; nnz == 0 or F == 0 zero-fills the results); NULL -> GESPMM_EINVAL; a 16-bit pointer not 2-byte aligned, delta
 * or the seed not 4-byte aligned, stats not 8-byte aligned -> GESPMM_EALIGN. No atomics, no workspace, no allocation, no host
 * synchronisation: capturable.
 */
int gespmm_dot_attention_x16(const int32_t* rowptr, const int32_t* colind, const void* q, const void* k, const void* v, void* out,
                             float* stats, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, void* stream);
int gespmm_dot_attention_dropout_x16(const int32_t* rowptr, const int32_t* colind, const void* q, const void* k, const void* v, void* out,
                                     float* stats, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, float p,
                                     const void* seed, void* stream);
int gespmm_dot_attention_backward_q_x16(const int32_t* rowptr, const int32_t* colind, const void* q, const void* k, const void* v,
                                        const float* stats, const void* out, const void* grad_out, float* delta, void* grad_q, int dtype,
                                        int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, void* stream);
int gespmm_dot_attention_backward_q_dropout_x16(const int32_t* rowptr, const int32_t* colind, const void* q, const void* k, const void* v,
                                                const float* stats, const void* out, const void* grad_out, float* delta, void* grad_q,
                                                int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, float p,
                                                const void* seed, void* stream);
int gespmm_dot_attention_backward_kv_x16(const int32_t* colptr, const int32_t* rowind, const void* q, const void* k, const void* v,
                                         const float* stats, const float* delta, const void* grad_out, void* grad_k, void* grad_v, int dtype,
                                         int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, void* stream);
int gespmm_dot_attention_backward_kv_dropout_x16(const int32_t* colptr, const int32_t* rowind, const void* q, const void* k, const void* v,
                                                 const float* stats, const float* delta, const void* grad_out, void* grad_k, void* grad_v,
                                                 int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float scale, float p,
                                                 const void* seed, void* stream);
/* Host only: what the three 16-bit entry points would launch, in the words of gespmm_describe_dot_attention. *_align: largest power of
 * two (>= 2) dividing the 16-bit operand's address (pass the least of the 16-bit results' with them); the answer is
 * gespmm_describe_dot_attention's at twice each alignment, capped at 16. Returns the length written or a GESPMM_E* code. */
int gespmm_describe_dot_attention_x16(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, int q_align, int k_align, int v_align,
                                      char* out, int64_t capacity);
/*
 * Fused GATv2 attention over the entries of a pattern — score, softmax and aggregation in ONE sweep — and its backward, with NOTHING of
 * size nnz but the index arrays (new symbols of 0.5). xl [M x H x F] is the aggregating node's term (the row of an entry), xr
 * [K x H x F] the neighbour's (the column), att [H x F]; out and grad_out [M x H x F], stats [M x H x 2], delta [M x H]. slope == 1:
 * no multiply. For entry p of row r with column c and head h
 *
 *     t_pf = fl(xl[r, h, f] + xr[c, h, f])      s_p = sum_f att[h, f] leaky(t_pf)      leaky(t) = t >= 0 ? t : fl(slope t)
 *     a_p = exp(s_p - m) / l,  (m, l) = stats[r, h] = (max_p s_p, sum_p exp(s_p - m))      out[r, h, :] = sum_p a_p xr[c, h, :]
 *
 * The neighbour's slice is the score's operand AND the aggregated value: one gathered row per entry serves the forward. Geometry of
 * all three kernels: that of gespmm_dot_attention_f32 — a group of W lanes owns a (segment, head) pair (rows in the forward and in
 * _backward_row, columns in _backward_col) with V floats per load and 8 floats per lane and operand; (V, W) from
 * gespmm_describe_gatv2_attention: V the widest of 4 / 2 / 1 that divides F and whose bytes divide the address of every dense operand
 * (xl, xr, att and the dense results), W the smallest power of two in 4 .. 64 with 8 W >= F — the rule of gespmm_describe_gatv2_score.
 * F > 512 is not served: GESPMM_ERR_UNSUPPORTED, nothing launched. A hub segment is walked by its one lane group (a limit).
 * Pinned orders: s_p is the lane chain acc = fmaf(att_j, leaky(fl(xl_j + xr_j)), acc) and xor butterfly of gespmm_gatv2_score_f32, so
 * on equally aligned operands it has that call's bits; dot(x, y) is the pinned dot of gespmm_dot_attention_f32. The fp32 add and fmaf
 * commute in their factors: both backward passes see the same bits of t, s_p and g_p. Every per-word accumulation is one chain per
 * output word in segment (entry) order.
 *
 * Forward — one sweep with the online softmax of gespmm_dot_attention_f32 (the same per-entry expressions with v = xr, the same first
 * entry, out = acc / l). Every word of out and stats is written; an empty row writes +0 everywhere.
 * gespmm_gatv2_attention_backward_row_f32 (rowptr, colind) writes delta, grad_xl and — unless att_part is NULL — att_part [M x H x F]:
 *     delta[r, h] = dot(grad_out[r, h, :], out[r, h, :])     g_p = dot(grad_out[r, h, :], xr[c, h, :])     ds_p = a_p (g_p - delta[r, h])
 *     m_pf = t_pf >= 0 ? att[h, f] : fl(att[h, f] slope)                                        with a_p = __expf(s_p - m) / l
 *     grad_xl[r, h, f] = chain over p of fmaf(ds_p, m_pf, acc)          att_part[r, h, f] = chain over p of fmaf(ds_p, leaky(t_pf), acc)
 * (grad_att is att_part summed over r by the caller).
 * gespmm_gatv2_attention_backward_col_f32 (colptr, rowind: the CSC arrays, no csc_order) reads delta and writes
 *     grad_xr[c, h, f] = fl( chain over p of fmaf(ds_p, m_pf, acc1) + chain over p of fmaf(a_p, grad_out[r, h, f], acc2) )
 * The *_dropout_f32 forms put dropout on a_p (the mask of gespmm_edge_dropout_f32: a function of (seed, r, c, h)) where
 * gespmm_dot_attention_dropout_f32 puts it: the forward's l sums every entry and acc takes fl(t s) for a kept entry, +0 for a dropped
 * one; the backward replaces g_p by fl(g_p s) or +0 directly after its chain, delta stays dot(grad_out, out), the second chain of
 * grad_xr uses fl(a_p s) or +0.
 * Checks, in this order: a negative size, H < 1, M < 1 or K < 1 with nnz > 0, a NaN or infinite slope, !(0 <= p < 1) -> GESPMM_EINVAL;
 * M, K, nnz, nnz H, M H F, K H F or 2 M H > 2^31 - 4097 -> GESPMM_ERANGE; F > 512 -> GESPMM_ERR_UNSUPPORTED; nnz == 0 or F == 0 looks at
 * the results (and the seed) alone and zero-fills them (hipMemsetAsync); NULL (att_part excepted) -> GESPMM_EINVAL; a pointer not
 * 4-byte (stats: 8-byte) aligned -> GESPMM_EALIGN. No atomics, no workspace, no allocation, no host synchronisation: capturable.
 * Results must not overlap an input (not checked); xl and xr may be the same array. colind within [0, K), rowind within [0, M) and
 * ptr[last] == nnz are preconditions.
 */
int gespmm_gatv2_attention_f32(const int32_t* rowptr, const int32_t* colind, const float* xl, const float* xr, const float* att, float* out,
                               float* stats, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, void* stream);
int gespmm_gatv2_attention_dropout_f32(const int32_t* rowptr, const int32_t* colind, const float* xl, const float* xr, const float* att,
                                       float* out, float* stats, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope,
                                       float p, const void* seed, void* stream);
int gespmm_gatv2_attention_backward_row_f32(const int32_t* rowptr, const int32_t* colind, const float* xl, const float* xr, const float* att,
                                            const float* stats, const float* out, const float* grad_out, float* delta, float* grad_xl,
                                            float* att_part, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope,
                                            void* stream);
int gespmm_gatv2_attention_backward_row_dropout_f32(const int32_t* rowptr, const int32_t* colind, const float* xl, const float* xr,
                                                    const float* att, const float* stats, const float* out, const float* grad_out,
                                                    float* delta, float* grad_xl, float* att_part, int64_t M, int64_t K, int64_t H,
                                                    int64_t F, int64_t nnz, float slope, float p, const void* seed, void* stream);
int gespmm_gatv2_attention_backward_col_f32(const int32_t* colptr, const int32_t* rowind, const float* xl, const float* xr, const float* att,
                                            const float* stats, const float* delta, const float* grad_out, float* grad_xr, int64_t M,
                                            int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, void* stream);
int gespmm_gatv2_attention_backward_col_dropout_f32(const int32_t* colptr, const int32_t* rowind, const float* xl, const float* xr,
                                                    const float* att, const float* stats, const float* delta, const float* grad_out,
                                                    float* grad_xr, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope,
                                                    float p, const void* seed, void* stream);
/* Host only: what the three entry points would launch, as text: "V=.. W=.. supported=1", "route=unsupported supported=0" (F > 512),
 * "route=zeros supported=1" (F == 0) or "form=none supported=1" (nnz == 0). *_align: largest power of two (>= 4) dividing the operand's
 * address (pass the least of the dense results' with xl's); the least of them decides V. Returns the length written or a GESPMM_E* code. */
int gespmm_describe_gatv2_attention(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, int xl_align, int xr_align, int att_align,
                                    char* out, int64_t capacity);
/*
 * ... on 16-bit node terms (new symbols of 0.5): xl, xr, out, grad_out, grad_xl and grad_xr are IEEE fp16 or bfloat16 (dtype:
 * GESPMM_X16_F16 / GESPMM_X16_BF16, one type per call); att, stats, delta and att_part stay fp32 — parameters, row statistics and
 * everything a sum over nodes is taken of, the split of gespmm_gatv2_score_x16.
 * The arithmetic is the fp32 contract above, expression for expression: every 16-bit element is widened exactly at its use (subnormals
 * included), t = fl32(widen(xl_j) + widen(xr_j)) is ONE fp32 add, the leaky branch is t >= 0; the score chain, the pinned dot, the xor
 * butterfly and the online softmax are the fp32 kernel's; every accumulation is fp32, in entry order. _backward_row reads the STORED,
 * 16-bit out for delta = dot(grad_out, out). Every 16-bit result is rounded ONCE, at its store (to nearest even, overflow to +-inf, NaN
 * stays NaN); for grad_xr that is the one add of its two chains, then one rounding. No packed-fp16 arithmetic and no dot2.
 * Geometry (gespmm_describe_gatv2_attention_x16): the fp32 kernel's with V counted in ELEMENTS — V in {4, 2, 1}, an 8 / 4 / 2-byte load
 * of the 16-bit operands with att's V floats at the same positions; 8 elements per lane and operand; W the smallest power of two in
 * 4 .. 64 with 8 W >= F; V the widest of 4 / 2 / 1 that divides F, whose 2 V bytes divide the address of every 16-bit dense operand and
 * result and whose 4 V bytes divide the addresses of att and att_part. A 16-byte load form (V = 8) is deliberately not built.
 * Lane positions, chains and orders are those of the fp32 kernels at the same (V, W): wherever gespmm_describe_gatv2_attention answers
 * the same (V, W) for the widened operands (a 16-bit operand b bytes off a 16-byte boundary corresponds to an fp32 operand 2 b bytes
 * off), stats, delta and att_part have the BITS of the fp32 entry points on the widened operands — _backward_row fed widen(out),
 * _backward_col fed that delta — and out, grad_xl and grad_xr are those calls' results narrowed once.
 * Checks, in this order: a dtype that is neither code -> GESPMM_EINVAL; then the fp32 ladder with limits in ELEMENT positions (M H F,
 * K H F, nnz, nnz H, 2 M H <= 2^31 - 4097 -> else GESPMM_ERANGE; F > 512 -> GESPMM_ERR_UNSUPPORTED; nnz == 0 or F == 0 zero-fills the
 * results); NULL (att_part excepted) -> GESPMM_EINVAL; a 16-bit pointer not 2-byte aligned, att, delta or att_part not 4-byte aligned,
 * stats not 8-byte aligned -> GESPMM_EALIGN. xl and xr may be the same array. No atomics, no workspace, no allocation, no host
 * synchronisation: capturable.
 */
int gespmm_gatv2_attention_x16(const int32_t* rowptr, const int32_t* colind, const void* xl, const void* xr, const float* att, void* out,
                               float* stats, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, void* stream);
int gespmm_gatv2_attention_dropout_x16(const int32_t* rowptr, const int32_t* colind, const void* xl, const void* xr, const float* att,
                                       void* out, float* stats, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz,
                                       float slope, float p, const void* seed, void* stream);
int gespmm_gatv2_attention_backward_row_x16(const int32_t* rowptr, const int32_t* colind, const void* xl, const void* xr, const float* att,
                                            const float* stats, const void* out, const void* grad_out, float* delta, void* grad_xl,
                                            float* att_part, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, float slope,
                                            void* stream);
int gespmm_gatv2_attention_backward_row_dropout_x16(const int32_t* rowptr, const int32_t* colind, const void* xl, const void* xr,
                                                    const float* att, const float* stats, const void* out, const void* grad_out,
                                                    float* delta, void* grad_xl, float* att_part, int dtype, int64_t M, int64_t K, int64_t H,
                                                    int64_t F, int64_t nnz, float slope, float p, const void* seed, void* stream);
int gespmm_gatv2_attention_backward_col_x16(const int32_t* colptr, const int32_t* rowind, const void* xl, const void* xr, const float* att,
                                            const float* stats, const float* delta, const void* grad_out, void* grad_xr, int dtype, int64_t M,
                                            int64_t K, int64_t H, int64_t F, int64_t nnz, float slope, void* stream);
int gespmm_gatv2_attention_backward_col_dropout_x16(const int32_t* colptr, const int32_t* rowind, const void* xl, const void* xr,
                                                    const float* att, const float* stats, const float* delta, const void* grad_out,
                                                    void* grad_xr, int dtype, int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz,
                                                    float slope, float p, const void* seed, void* stream);
/* Host only: what the three 16-bit entry points would launch, in the words of gespmm_describe_gatv2_attention. xl_align, xr_align:
 * largest power of two (>= 2) dividing the 16-bit operands' addresses (pass the least of the 16-bit results' with them); att_align
 * (>= 4): the least of att and att_part. Returns the length written or a GESPMM_E* code. */
int gespmm_describe_gatv2_attention_x16(int64_t M, int64_t K, int64_t H, int64_t F, int64_t nnz, int xl_align, int xr_align, int att_align,
                                        char* out, int64_t capacity);
/* New values on the unchanged pattern (val in the caller's CSR order, device memory; NULL = A == 1). */
int gespmm_plan_set_values(gespmm_plan* plan, const float* val, void* stream);
/* perm_host[i] = row processed at position i (HOST memory, M entries). Returns 1 if clustered, 0 if storage order. */
int gespmm_plan_get_order(const gespmm_plan* plan, int32_t* perm_host);
/* One line of text: order, cluster hierarchy, tasks, modelled L2 hit rate before -> after, analysis time, launch. */
int gespmm_plan_describe(const gespmm_plan* plan, char* out, int64_t capacity);
void gespmm_plan_destroy(gespmm_plan* plan);
/* The analysis stage keeps its scratch arena for the next plan — one per device, up to a limit of 1 GiB by default
 * (GESPMM_ARENA_CACHE_MB overrides the default; a products-sized analysis takes ~10 GB, freed when the plan is made unless the
 * limit says otherwise). gespmm_set_cached_memory_limit changes the limit (bytes; negative = default), gespmm_release_cached_memory
 * gives the kept arenas back. */
void gespmm_set_cached_memory_limit(int64_t bytes);
void gespmm_release_cached_memory(void);

/*
 * Warm-up (since 0.3). The FIRST plan a process builds pays ~29 ms on top of its analysis: the analysis kernels are loaded on first use
 * and the scratch arena is allocated (profiles/r06/plan_cold.log). A process that follows the reference's protocol — one process per
 * matrix, 200 launches (run_test.sh:5-11) — cannot amortise that, so the driver and the Python layer call gespmm_init before they time
 * anything: it builds and destroys plans on a small built-in matrix (every analysis pass, the staging tables, one product through each
 * kernel family) and reserves the arena a matrix of (rows_hint, nnz_hint) will ask for (0 / 0: nothing reserved; within the limit of
 * gespmm_set_cached_memory_limit). Idempotent per device; returns 0 or an error code. Until it (or a first plan) has run, a plan made
 * with reorder = AUTO adds the cold cost to its cost rule (gespmm_plan_policy_query.cold_start).
 */
int gespmm_init(int64_t rows_hint, int64_t nnz_hint, void* stream);
/* 1 if an analysis of a matrix of this shape could pay for itself inside `expected_launches` (0 = 200) products once the library is warm
 * (the cost rule with the most structure a probe can report), else 0: for such a matrix there is nothing to warm up for — a plan keeps
 * its storage order either way. Host only. The Python layer asks this before it spends gespmm_init's ~60 ms on a pubmed-sized graph. */
int gespmm_plan_wants_warmup(int64_t M, int64_t K, int64_t nnz, int64_t N, int32_t expected_launches);

/*
 * Plan reuse behind the STATELESS entry points (since 0.3; off by default). The reference's callers keep no state between products
 * (spmmWrapper spmm_test.cu:456-492, spmm_cuda spmm_kernel.cu:425-458, DGL's CustomCsrmm binary_reduce_sum.cu:338-360), so they cannot
 * hold a gespmm_plan. gespmm_set_auto_plan(k), k >= 1: gespmm_csr_spmm_f32, gespmm_csr_spmm_max_f32 and gespmm_dgl_csrmm_{sum,max}_f32
 * keep a small cache (8 entries, least recently used) keyed on (device, stream, rowptr, colind, M, K, N, valued, variant, reducer); the k-th
 * call with one key builds a plan (synchronously), later calls run through it. Pointer identity is not pattern identity: every call
 * that uses a cached plan first fingerprints ALL of rowptr / colind / val on the device (one small kernel + a 32-byte read-back = one
 * stream synchronisation per call — the price of the switch: ~25 us on a com-Amazon-sized graph, where the plan saves ~60). A pattern
 * changed in place drops the plan, changed values are re-permuted. Where the plan's launch and the plain launch are one kernel each (no
 * long-row pass, no cache blocking) the calls after the plan's creation do not synchronise at all: the fingerprint is compared ON THE
 * DEVICE, the plan's kernel and the plain kernel are both enqueued behind the result (one of them runs, the other's workgroups leave at
 * once), and the host learns of a change from a record the check leaves in pinned memory, at the next call. Never on a capturing stream. Matrices whose analysis keeps the
 * storage order run the plain path without fingerprint from then on. Results: the plain call's bits for the operands as they are at
 * that point in STREAM order, on any number of streams, whether or not the host waited for in-place changes that are ordered on the
 * stream. The stream is part of the key, so each stream keeps its own plan and device-side check state (a plan per stream
 * and graph: two streams on one graph take two of the 8 entries and twice the plan memory); a record of changed values is never
 * adopted — the call that reads it re-fingerprints synchronously and re-permutes from that; the check state is zeroed whenever a plan
 * is made; the record is a seqlock (round-6 advisor findings 1-3).
 * k = 0 switches it off and frees the cached plans; gespmm_auto_plan_clear frees them and keeps the switch.
 */
typedef struct gespmm_auto_plan_stats {
    int64_t calls_planned;     /* products that ran through a cached plan */
    int64_t plans_created;
    int64_t invalidated;       /* plans dropped because the pattern's fingerprint changed */
    int64_t values_refreshed;  /* gespmm_plan_set_values calls after the values' fingerprint changed */
    int64_t fingerprints;      /* fingerprint passes (= stream synchronisations the switch added) */
    int64_t cached_plans;      /* plans alive now */
    int64_t calls_async;       /* of calls_planned: launched behind a device-side guard, without any synchronisation (see above) */
} gespmm_auto_plan_stats;
int gespmm_set_auto_plan(int32_t kth_call);
void gespmm_auto_plan_clear(void);
int gespmm_auto_plan_get_stats(gespmm_auto_plan_stats* out);

/*
 * The clustering by itself, HOST pointers (what gespmm_plan_create runs on its host copy): multi-level label
 * propagation on the bipartite row/column graph; perm_out[i] = row at position i. Deterministic, independent of
 * `threads`. levels_out / clusters_out[16] (row clusters after each level) may be NULL.
 */
int gespmm_cluster_rows(const int32_t* rowptr, const int32_t* colind, int64_t M, int64_t K, int32_t threads,
                        int32_t* perm_out, int32_t* levels_out, int32_t* clusters_out);
/* Study hook (scripts/cluster_chain_study.py; HOST pointers): the same clustering with its depth / sweeps given, plus the coarsest
 * cluster of every row (top_label_out[M], may be NULL). Returns the number of levels built or a negative error. */
int gespmm_cluster_rows_study(const int32_t* rowptr, const int32_t* colind, int64_t M, int64_t K, int32_t max_levels, int32_t sweeps,
                              int32_t* perm_out, int32_t* top_label_out, int32_t* clusters_out);
/*
 * Model of the per-XCD L2 used to judge an order (HOST pointers): rows processed in `perm` order (NULL = storage
 * order) in `slices` contiguous parts of equal non-zero count, each with an LRU of `window_rows` B rows; returns
 * the share of non-zeros whose B row is resident when gathered.
 */
double gespmm_simulate_l2_hits(const int32_t* rowptr, const int32_t* colind, int64_t M, int64_t K, const int32_t* perm,
                               int32_t slices, int64_t window_rows);

/*
 * The device analysis passes by themselves (what gespmm_plan_create runs; DEVICE rowptr / colind, HOST outputs):
 * gespmm_device_cluster_rows gives the SAME order as gespmm_cluster_rows (the rules are identical and every sum is an
 * integer sum); gespmm_device_l2_model estimates what gespmm_simulate_l2_hits simulates (exact LRU stack distances of
 * `samples_per_slice` stratified accesses per slice; max_entries_per_slice > 0 models only the head of every slice).
 */
int gespmm_device_cluster_rows(const int32_t* rowptr, const int32_t* colind, int64_t M, int64_t K, int64_t nnz,
                               int32_t* perm_out_host, int32_t* levels_out, int32_t* clusters_out, void* stream);
double gespmm_device_l2_model(const int32_t* rowptr, const int32_t* colind, int64_t M, int64_t K, int64_t nnz,
                              const int32_t* perm_host, int32_t slices, int64_t window_rows, int64_t max_entries_per_slice,
                              int32_t samples_per_slice, void* stream);
/* Test hook: task table of a clustered plan (which = 0 wavefront tasks, 1 lane-group tasks), int4 records, HOST memory. */
int gespmm_plan_debug_tasks(const gespmm_plan* plan, int32_t which, int32_t* out_host, int64_t capacity);
/* Test hook: the staging lists of a plan's staged-rows tables — blocks x slots column indices (-1: slot not used), HOST memory; info_host =
 * {blocks, slots per block, rows per block, window of the fill pass (0: none)}. Returns blocks * slots (<= capacity words are copied), 0 without such tables. */
int64_t gespmm_plan_debug_staging(const gespmm_plan* plan, int32_t* info_host, int32_t* out_host, int64_t capacity);

/*
 * The plan's POLICY by itself (host only, no device, no matrix): what gespmm_plan_create / gespmm_plan_spmm_f32 decide for a
 * matrix of this shape once the analysis has produced the numbers in the query (csrc/plan_policy.cpp holds the rules, each
 * with the log it was measured in). Lets callers and tests ask "what would a plan do" without building one.
 */
typedef struct gespmm_plan_policy_query {
    int64_t M, K, nnz, N;
    int64_t N_launch;        /* width of the launch asked about (0 = N) */
    int32_t variant;         /* GESPMM_VARIANT_* */
    int32_t max_degree;      /* longest row */
    int32_t reorder, kernel, analysis, flags, task_entries, row_floor; /* as in gespmm_plan_options */
    double hits_before, hits_after; /* modelled L2 hit rates in storage / clustered order */
    double staged_fraction;  /* share of the entries whose B row a staged-rows block holds in LDS */
    /* since 0.3 (read by gespmm_plan_policy_v2 when q_bytes covers them) */
    int32_t expected_launches; /* as in gespmm_plan_options (0 = 200) */
    int32_t cold_start;        /* since 0.3: 1 = the process has built no plan and gespmm_init has not run — the first analysis also loads
                                  its kernels and makes its arena (~29 ms): the cost rule is asked with that on top */
    double wedge_probe;      /* share of sampled (row r; c1, c2 in r) wedges with c2 in row c1 — the plan's cheap structure probe on square
                                matrices; negative = unknown (rectangular matrix, host analysis) */
    double record_slot_fill; /* padded-record kernel (round 6, read when q_bytes covers it): share of the batches' entry slots that carry an
                                entry once its tables are built; negative = not known yet (keep_records then repeats build_records) */
} gespmm_plan_policy_query;
typedef struct gespmm_plan_policy_answer {
    int32_t launch_flags;      /* user flags + GESPMM_FLAG_SPLIT_LONG_ROWS or _STRICT_ORDER */
    int32_t analyse;           /* clustering + L2 model run at all */
    int32_t dense_try;         /* dense graph: the clustered order needs >= 0.65 modelled hits */
    int32_t keep_clustered;    /* ... and is kept, given hits_before / hits_after */
    int32_t task_entries, group_task_entries, row_floor;
    int32_t build_staged, keep_staged; /* staged-rows tables are built / kept, given staged_fraction */
    int32_t shallow_unroll;
    int32_t segmented;         /* the streaming launch at N_launch takes the segmented-stream kernel */
    int32_t sddmm_route;       /* 0 CSR call, 1 COO on expanded row ids, 2 clustered edge order + scatter */
    int32_t narrow_vec4;       /* the launch at N_launch <= 64 takes 4 floats per lane (variant 3) instead of 1 */
    int64_t model_window, model_sample;
    /* since 0.3 (written by gespmm_plan_policy_v2 when a_bytes covers them) */
    int32_t cost_skipped;      /* reorder = AUTO would have analysed, but gain x launches < cost: storage order, no analysis */
    int32_t cluster_levels;    /* clustering depth of this plan (0 = the clustering's own default: six levels) */
    double est_gain_us;        /* estimated saving per launch if the clustered order is kept */
    double est_cost_us;        /* estimated time of the analysis */
    int32_t cluster_sweeps;    /* label-propagation sweeps per level (0 = the clustering's own default: five) */
    int32_t staged_rows;       /* rows per block of the staged-rows tables at this width (0: the width is not served) */
    /* round 6 (written when a_bytes covers them): the padded-record kernel (GESPMM_PLAN_KERNEL_RECORDS) */
    int32_t build_records, keep_records; /* its tables are built (clustered order kept, narrow width, short rows, no staged tables kept) /
                                            kept, given record_slot_fill */
    int32_t records_batches;   /* batches a wavefront task of those tables is cut at */
    int32_t slab_ranges;       /* column-slab tables (GESPMM_PLAN_KERNEL_STAGED_SLABS): ascending column ranges the plan cuts its clustered matrix
                                  into at this width — 0: no such tables (kept once >= 50 % of the entries find their B row staged) */
    int32_t staged_fill_window; /* fill pass of the staged-rows tables (written when a_bytes covers it): free slots of a block go to columns it
                                   uses once whose own row lies within this many blocks in the plan's order — 0: no fill pass */
} gespmm_plan_policy_answer;
int gespmm_plan_policy(const gespmm_plan_policy_query* q, gespmm_plan_policy_answer* a);  /* the 0.2 layouts (up to staged_fraction / model_sample) */
int gespmm_plan_policy_v2(const gespmm_plan_policy_query* q, int64_t q_bytes, gespmm_plan_policy_answer* a, int64_t a_bytes);

/*
 * Comparison column, not a product path: the Gunrock app's edge map
 * (gunrock-test/app/spmm/spmm_enactor.cuh:92-105) — for every edge (src -> dest) of the CSR pattern
 * and every feature j, atomicAdd(out + dest*N + j, in[src*N + j]): out[K x N] = A^T * in with A == 1,
 * `out` zeroed by the call. `in` is M x N. The order of the additions is not fixed (atomics), so
 * results are tolerance-checked. spmm_test --atomic-baseline times it next to the row-product kernels.
 */
int gespmm_baseline_atomic_scatter_f32(const int32_t* rowptr, const int32_t* colind, const float* in, float* out,
                                       int64_t M, int64_t K, int64_t N, int64_t nnz, void* stream);

/*
 * Yardstick, not a product path: dst[i] = src[i] for n floats as one streaming kernel (dwordx4 per lane where both
 * pointers are 16-byte aligned). bench.py times it in the same process as the product, so that `roofline.ceiling_frac`
 * is priced with the read + write rate of the box the product ran on (no reference counterpart: the reference reports
 * GFLOP/s only, spmm_test.cu:728-738).
 */
int gespmm_baseline_copy_f32(const float* src, float* dst, int64_t n, void* stream);

/* ------------------------------------------------------------------ host side */

/*
 * MatrixMarket coordinate loader with the reference's readMtx semantics
 * (1-based -> 0-based, `symmetric` expanded with self-loops and duplicates
 * dropped, result sorted by (row, col); real -> value, integer -> value,
 * pattern -> 1.0). Output arrays are HOST memory allocated by the library;
 * release them with gespmm_mtx_free(). Unlike the reference this never exits:
 * a missing file is GESPMM_EIO, a bad banner/size line GESPMM_EFORMAT.
 */
typedef struct gespmm_coo {
    int32_t  nrows;
    int32_t  ncols;
    int64_t  nnz;
    int32_t* row;   /* [nnz] */
    int32_t* col;   /* [nnz] */
    float*   val;   /* [nnz] */
} gespmm_coo;

int  gespmm_mtx_read(const char* path, gespmm_coo* out);
void gespmm_mtx_free(gespmm_coo* coo);

/*
 * Same result through a binary cache: the parsed, expanded and sorted COO of `path`
 * is stored as `<cache_dir>/<basename>.<bytes>.<mtime>.gespmm-coo` on the first read
 * and read back (one fread per array) afterwards; a changed file gets a new cache
 * name. cache_dir == NULL behaves like gespmm_mtx_read. (The reference re-parses the
 * text with fscanf on every run, util.hpp:104-216 — seconds for 10^7-entry files.)
 */
int  gespmm_mtx_read_cached(const char* path, const char* cache_dir, gespmm_coo* out);

/*
 * COO (any order) -> CSR by counting sort on the row, keeping the input order
 * inside each row. val_in == NULL writes 1.0f for every entry, which is what
 * spmm_test.cu:574 does with the file's values. All HOST pointers. An index
 * outside [0,nrows) x [0,ncols) is GESPMM_EINVAL (the reference only prints
 * "out of bound row/column", spmm_test.cu:563,571, and corrupts memory).
 */
int gespmm_coo_to_csr(int32_t nrows, int32_t ncols, int64_t nnz,
                      const int32_t* row, const int32_t* col, const float* val_in,
                      int32_t* rowptr, int32_t* colind, float* val_out);

/*
 * 1-D row partition of a CSR matrix into `parts` contiguous row ranges with
 * (nearly) equal non-zero counts: cut[p] = first row of part p, cut[parts] = M.
 * rowptr is HOST memory (M+1 entries); cut has parts+1 entries.
 */
int gespmm_row_partition(const int32_t* rowptr, int64_t M, int32_t parts, int64_t* cut);

#ifdef __cplusplus
}
#endif
#endif /* GESPMM_H_ */
