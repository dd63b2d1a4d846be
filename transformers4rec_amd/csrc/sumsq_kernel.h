// The sum of squares of a float buffer in double: ONE thread body and ONE reduction order for every entry point that runs it
// (optim.hip: t4r_grad_sumsq over a flat bucket; row_adam.hip: t4r_row_adam_reduce over the compact rows of a table).
#pragma once
#include "t4r_common.h"

#define T4R_SUMSQ_MAX_PARTS 2048      // 256 CUs x 8 workgroups: the grid of a memory-bound kernel; the rest is grid-stride

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// the four waves' sums in wave order; valid in thread 0
__device__ __forceinline__ double block_sum_d(double v) {
    __shared__ double sh[4];
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}
__device__ __forceinline__ double sq4(double acc, const float4 x) {
    acc = fma((double)x.x, (double)x.x, acc);
    acc = fma((double)x.y, (double)x.y, acc);
    acc = fma((double)x.z, (double)x.z, acc);
    return fma((double)x.w, (double)x.w, acc);
}

// the number of workgroups (= partials) of a launch over n elements
static inline long sumsq_parts(long n) {
    if (n <= 0) return 0;
    long blocks = (n / 4 + 255) / 256;
    if (blocks > T4R_SUMSQ_MAX_PARTS) blocks = T4R_SUMSQ_MAX_PARTS;
    return blocks < 1 ? 1 : blocks;
}

// A streaming read: 4 bytes per element and one double multiply-add, so HBM is the roof.  Squares and sums are in double from
// the element up -- (double)g * (double)g is exact, 1e18 does not overflow and 1e-30 does not vanish as their fp32 squares do,
// and the sum of n <= 2^31 non-negative terms is good to n * 2^-53 relative in any order.  The order is nevertheless fixed
// (a thread's elements in address order, the butterfly over the wave, the four waves in order): same bits on every run.
// Four independent 16-byte loads are in flight per thread while a full group of four trips remains.
// -> the workgroup's sum over its elements of g[0, n), valid in thread 0; 0.0 for a workgroup whose elements all lie past n.
// g is 16-byte aligned; every thread of the workgroup calls it with i = its first element, 4 * its global index, and stride =
// 4 * the threads of the grid (sumsq_first / sumsq_stride: the kernel evaluates them, where the compiler knows the launch bounds).
#define sumsq_first() (((long)blockIdx.x * blockDim.x + threadIdx.x) * 4)
#define sumsq_stride() ((long)gridDim.x * blockDim.x * 4)
__device__ __forceinline__ double sumsq_block(const float* __restrict__ g, long n, long i, const long stride) {
    double acc = 0.0;
    for (; i + 3 * stride + 4 <= n; i += 4 * stride) {
        const float4 a = *reinterpret_cast<const float4*>(g + i);
        const float4 b = *reinterpret_cast<const float4*>(g + i + stride);
        const float4 c = *reinterpret_cast<const float4*>(g + i + 2 * stride);
        const float4 d = *reinterpret_cast<const float4*>(g + i + 3 * stride);
        acc = sq4(sq4(sq4(sq4(acc, a), b), c), d);
    }
    for (; i < n; i += stride) {
        if (i + 4 <= n) {
            acc = sq4(acc, *reinterpret_cast<const float4*>(g + i));
        } else {
            for (long j = i; j < n; ++j) acc = fma((double)g[j], (double)g[j], acc);
        }
    }
    return block_sum_d(acc);
}
