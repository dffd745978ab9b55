// spmm_max_arg.hip — the max reducer with argmax and its gradient (spmm_max_arg.h): the batch-stream kernel of spmm_stream.h with a
// position register next to every accumulator word (forward), and the same walk over CSC columns that compares the saved positions
// and adds grad_out where they match (backward). A translation unit of its own: the kernels of spmm_stream.h stay exactly what they are.
// The kernel body stands in spmm_max_arg_kernel.h, a template on the element type that spmm_max_arg_x16.hip shares; these are its
// fp32 instantiations (DT = 0), whose gfx950 instruction text is what it was when the body stood here.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spmm_device.h"
#include "spmm_max_arg.h"
#include "spmm_max_arg_kernel.h"

namespace gespmm {

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
    hipLaunchKernelGGL((max_arg_kernel_t<0, V, S, W, U, BACKWARD>), dim3((unsigned)nitems), dim3(kThreads), 0, st, args);
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
