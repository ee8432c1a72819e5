// The fixed-order reductions of the loss, decode and metric kernels (64-lane waves, workgroups of four).  Nothing but additions,
// comparisons and shuffles: no multiply, so files that differ in their fp-contraction setting share them.
#pragma once
#include "common.h"

namespace mp {

// xor butterfly 32 ... 1: the sum of the wave's 64 values, the same bits in every lane
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// (w0 + w1) + (w2 + w3) of a four-wave workgroup, v being a wave_sum.  Valid in thread 0 only; holds a barrier.
template <typename T>
__device__ __forceinline__ T block_sum_lane0(T v, T* ws4) {
    if ((threadIdx.x & 63) == 0) ws4[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) v = (ws4[0] + ws4[1]) + (ws4[2] + ws4[3]);
    return v;
}

// sum of one value per thread over a four-wave workgroup, the same value in every thread
template <typename T>
__device__ __forceinline__ T block_sum_all(T v, T* ws4) {
    v = wave_sum(v);
    __syncthreads();  // ws4 may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) ws4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (ws4[0] + ws4[1]) + (ws4[2] + ws4[3]);
}

// 256-slot LDS tree of a 256-thread workgroup: slot t takes slot t + s for s = 128 ... 1.  Leaves the sum in sm[0], behind a barrier.
__device__ __forceinline__ void block_tree_sum_256(double v, double (&sm)[256]) {
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
}

// the larger value wins, the smaller index among equals
__device__ __forceinline__ void argmax_combine(float& best, int& bidx, float ov, int oi) {
    if (ov > best || (ov == best && oi < bidx)) {
        best = ov;
        bidx = oi;
    }
}

// xor butterfly of argmax_combine: the wave's arg-max in every lane
__device__ __forceinline__ void wave_argmax(float& best, int& bidx) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bidx, off, 64);
        argmax_combine(best, bidx, ov, oi);
    }
}

}  // namespace mp
