// spmm_max_arg.h — internal interface of the max reducer WITH ARGMAX and of its gradient (gespmm_csr_spmm_max_arg_f32 /
// gespmm_csr_spmm_max_backward_f32; kernels: spmm_max_arg.hip).
//
// Forward, one sequential chain per output word (r, c) — the contract, whatever the lane geometry:
//   acc = empty; a = -1;  for p = rowptr[r] .. rowptr[r + 1] - 1 ascending: b = B[colind[p] N + c]; if (b > acc) { acc = b; a = p; }
//   C[r, c] = acc; arg[r, c] = a                       (a CSR POSITION; first of equal values, +0 == -0, NaN never wins)
// Backward, for node k and column c, over the CSC arrays of the pattern (CSC position q is CSR entry order[q]):
//   g = +0;  for q = colptr[k] .. colptr[k + 1] - 1 ascending: r = rowind[q]; if (arg[r N + c] == order[q]) g = g + grad_out[r N + c]
//   grad_B[k, c] = g                                   (one plain fp32 add chain in CSC order; no atomics)
//
// Both kernels are the batch-stream walk of spmm_stream.h (spmm_heads.hip is the sibling): a wavefront owns `rpw` consecutive segments
// = one contiguous range of the index array, tiles of 64 entries staged in LDS one tile ahead, W lanes per segment with V floats per
// lane and S strips, U gathers back to back and one predicated tail group, 32-bit byte offsets. A segment is never split over lanes,
// so the chains above are what every lane runs. They exist in the batch-stream geometries select.cpp reaches without launch knobs:
//   V = 1: W = 4 .. 64 · V = 4: W = 32, 64 and two strips at W = 64 · V = 2 at W = 64 (one or two strips) · V = 1 with two strips at W = 64
// `order` and `arg` VALUES are trusted (they are compared, never used as an address); colind / rowind are trusted to be in range, as
// everywhere in this library.
#pragma once
#include "spmm_kernels.h"

namespace gespmm {

struct MaxArgArgs {
    const int32_t* ptr;     // forward: rowptr [M + 1] · backward: colptr [K + 1]
    const int32_t* ind;     // forward: colind · backward: rowind
    const int32_t* order;   // backward: CSC position -> CSR position
    const float* src;       // forward: B [K, N] · backward: grad_out [M, N]
    const int32_t* arg_in;  // backward: arg [M, N]
    float* dst;             // forward: C [M, N] · backward: grad_B [K, N]
    int32_t* arg_out;       // forward: arg [M, N]
    int32_t S;              // segments: M forward, K backward
    int32_t N;
    int32_t nblk;           // segment blocks (filled in by the launcher)
    int32_t ntile;          // column tiles (filled in by the launcher)
    int32_t rpw;            // segments per wavefront (filled in by the launcher)
    float empty;            // forward: initial accumulator
};

inline bool max_arg_geometry_served(const Geometry& g) {
    if (g.idx64 || g.slab_blocked || g.split_long_rows) return false;
    const int V = g.vec, S = g.strips, W = g.group;
    if (W != 4 && W != 8 && W != 16 && W != 32 && W != 64) return false;
    if (S == 2) return W == 64 && (V == 1 || V == 2 || V == 4);
    if (S != 1) return false;
    if (V == 1) return true;
    if (V == 2) return W == 64;
    if (V == 4) return W >= 32;
    return false;
}

// hipErrorInvalidValue where the geometry is not served.
hipError_t launch_spmm_max_arg(const MaxArgArgs& a, const Geometry& geo, hipStream_t st);
hipError_t launch_spmm_max_backward(const MaxArgArgs& a, const Geometry& geo, hipStream_t st);

// The same on 16-bit dense operands (spmm_max_arg_x16.hip; dtype kX16F16 / kX16Bf16): src and dst are the 16-bit arrays, arg stays int32,
// N and the geometry count ELEMENTS. The chains above run in fp32 on the exactly widened elements, from `empty` as given; C and grad_B
// are narrowed once at the store, to nearest even.
hipError_t launch_spmm_max_arg_x16(const MaxArgArgs& a, int dtype, const Geometry& geo, hipStream_t st);
hipError_t launch_spmm_max_backward_x16(const MaxArgArgs& a, int dtype, const Geometry& geo, hipStream_t st);

}  // namespace gespmm
