// spmm_max_arg_x16.hip — the max reducer with argmax and its gradient on 16-bit dense operands (gespmm_csr_spmm_max_arg_x16 /
// gespmm_csr_spmm_max_backward_x16: IEEE fp16 / bfloat16 B, C, grad_out and grad_B; arg stays int32): the kernel body of
// spmm_max_arg_kernel.h instantiated on the two 16-bit element types, and its launch table. A translation unit of its own: the fp32
// kernels of spmm_max_arg.hip stay exactly what they are.
//
// A geometry here counts ELEMENTS: V per lane and strip, the 11 entries of max_arg_geometry_served, asked of the selector with the
// effective alignment min(2 * (alignment of the 16-bit arrays), alignment of arg) — a V-element vector is 2 V bytes of B / C / grad and
// 4 V bytes of arg. V = 1 serves any N and any 2-byte aligned address: there is no composition route and no scratch.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spmm_device.h"
#include "spmm_max_arg.h"
#include "spmm_max_arg_kernel.h"

namespace gespmm {

template <int DT, int V, int S, int W, bool BACKWARD>
static hipError_t launch_max_arg_x16(const MaxArgArgs& a, int rpw, hipStream_t st) {
    // gather depth: the fp32 table's (spmm_max_arg.hip). The forward's gathered vectors are half the registers, its accumulators and
    // positions are not; the backward's main gathers are the same arg words.
    constexpr int U = (V * S >= (BACKWARD ? 4 : 8)) ? 4 : 8;
    MaxArgArgs args;
    int64_t nitems = 0;
    if (!max_arg_launch_shape<V, S, W>(a, rpw, &args, &nitems)) return nitems <= 0 ? hipSuccess : hipErrorInvalidConfiguration;
    hipLaunchKernelGGL((max_arg_kernel_t<DT, V, S, W, U, BACKWARD>), dim3((unsigned)nitems), dim3(kThreads), 0, st, args);
    return hipGetLastError();
}

template <int DT, bool BACKWARD>
static hipError_t launch_max_arg_x16_geometry(const MaxArgArgs& a, const Geometry& g, hipStream_t st) {
#define GESPMM_MAX_ARG_X16(V_, S_, W_) \
    if (g.vec == V_ && g.strips == S_ && g.group == W_) return launch_max_arg_x16<DT, V_, S_, W_, BACKWARD>(a, g.rows_per_wave, st);
    GESPMM_MAX_ARG_X16(1, 1, 4)
    GESPMM_MAX_ARG_X16(1, 1, 8)
    GESPMM_MAX_ARG_X16(1, 1, 16)
    GESPMM_MAX_ARG_X16(1, 1, 32)
    GESPMM_MAX_ARG_X16(1, 1, 64)
    GESPMM_MAX_ARG_X16(4, 1, 32)
    GESPMM_MAX_ARG_X16(4, 1, 64)
    GESPMM_MAX_ARG_X16(4, 2, 64)
    GESPMM_MAX_ARG_X16(2, 1, 64)
    GESPMM_MAX_ARG_X16(2, 2, 64)
    GESPMM_MAX_ARG_X16(1, 2, 64)
#undef GESPMM_MAX_ARG_X16
    return hipErrorInvalidValue;
}

// a.src / a.dst are the 16-bit arrays (B and C forward, grad_out and grad_B backward); a.N counts elements.
hipError_t launch_spmm_max_arg_x16(const MaxArgArgs& a, int dtype, const Geometry& geo, hipStream_t st) {
    if (!max_arg_geometry_served(geo)) return hipErrorInvalidValue;
    if (dtype == kX16F16) return launch_max_arg_x16_geometry<kX16F16, false>(a, geo, st);
    if (dtype == kX16Bf16) return launch_max_arg_x16_geometry<kX16Bf16, false>(a, geo, st);
    return hipErrorInvalidValue;
}

hipError_t launch_spmm_max_backward_x16(const MaxArgArgs& a, int dtype, const Geometry& geo, hipStream_t st) {
    if (!max_arg_geometry_served(geo)) return hipErrorInvalidValue;
    if (dtype == kX16F16) return launch_max_arg_x16_geometry<kX16F16, true>(a, geo, st);
    if (dtype == kX16Bf16) return launch_max_arg_x16_geometry<kX16Bf16, true>(a, geo, st);
    return hipErrorInvalidValue;
}

}  // namespace gespmm
