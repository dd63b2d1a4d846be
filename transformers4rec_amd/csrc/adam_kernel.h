// The fused Adam step over a flat buffer: ONE element arithmetic and ONE kernel body for every entry point that runs it
// (elementwise.hip: t4r_adam_step, t4r_adam_step_amax; optim.hip: t4r_adamw_step).
#pragma once
#include "t4r_common.h"

// torch.optim.Adam (amsgrad=False, maximize=False): with step t (1-based)
//   g = grad (+ wd * p) ; m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2
//   p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// grad_scale multiplies grad first (1/world_size for the DP mean).  Optionally zeroes the grad.
// The two bias corrections 1 - b1^t and sqrt(1 - b2^t) are computed in DOUBLE on the host (from the float betas the ABI
// takes) and passed to the kernel rounded once to float: in fp32 `1.f - powf(b2, t)` is a cancellation of a rounded power --
// 6.7e-6 relative at t = 2, which put p tens of fp32 roundings away from an exact Adam step during the first steps
// (tests/test_adam_gpu.py counts them).
// One element's step.  Every multiply-add is written out as the fmaf it is meant to be: left to the compiler's contraction, the
// two instantiations of the kernel (and its float4 body and scalar tail) fused different pairs and rounded m, v and p differently
// -- the two entry points disagreed in the last bit from the second step on (tests/test_adam_gpu.py holds them to one arithmetic).
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, float step_size, float b1, float b2,
                                             float eps, float wd, float bc2_sqrt, float grad_scale) {
    const float gr = fmaf(wd, p, g * grad_scale);
    m = fmaf(b1, m, (1.f - b1) * gr);
    v = fmaf(b2, v, ((1.f - b2) * gr) * gr);
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = fmaf(-step_size, m / denom, p);
}
// EXT (t4r_adamw_step) adds two things in front of that arithmetic and nothing else:
//   * the clip coefficient: the gradient the step sees is (g * grad_scale) * coef -- two roundings, "average, then clip", as
//     torch.nn.utils.clip_grad_norm_ over the averaged gradient.  coef is read from device memory (the launch before this one wrote
//     it: no host read); a null pointer is a coefficient of 1, and x * 1.0f is x: the bits of the plain step.
//   * decoupled weight decay (torch.optim.AdamW's order): p *= decay_factor first, then the Adam update WITHOUT the wd * p term.
__device__ __forceinline__ void adamw_element(float& p, float g, float& m, float& v, float step_size, float b1, float b2, float eps,
                                              float wd, float bc2_sqrt, float grad_scale, float coef, int decoupled,
                                              float decay_factor) {
    if (decoupled) p *= decay_factor;
    adam_element(p, (g * grad_scale) * coef, m, v, step_size, b1, b2, eps, decoupled ? 0.f : wd, bc2_sqrt, 1.f);
}
// AMAX (round 6): the launch also leaves, per workgroup, the largest |p| AFTER the update among the elements [amax_lo, amax_hi)
// in amax_part[blockIdx.x] -- the tied item table's maximum, which the next step's head needs to position its fp16 images
// (csrc/head_split.hip: split_w_images_kernel reduces the <= 1024 partials) and used to get from a memset + a 21 us pass over
// the 51 MB the optimizer has just streamed.  Plain stores, one slot per workgroup (same-address atomics serialise).
template <bool AMAX, bool EXT>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v,
                                                    long n, float lr, float b1, float b2, float eps,
                                                    float wd, float bc1, float bc2_sqrt,
                                                    float grad_scale, int zero_grad, long amax_lo, long amax_hi,
                                                    float* __restrict__ amax_part, const float* __restrict__ clip_coef,
                                                    int decoupled, float decay_factor) {
    float mx = 0.f;
    const float step_size = lr / bc1;
    const float coef = EXT && clip_coef ? *clip_coef : 1.f;
    const long stride = (long)gridDim.x * blockDim.x * 4;
    for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
        if (i + 4 <= n) {
            float4 pp = *reinterpret_cast<float4*>(p + i);
            float4 gg = *reinterpret_cast<float4*>(g + i);
            float4 mm = *reinterpret_cast<float4*>(m + i);
            float4 vv = *reinterpret_cast<float4*>(v + i);
            float* P = &pp.x; float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (EXT) adamw_element(P[e], G[e], M[e], V[e], step_size, b1, b2, eps, wd, bc2_sqrt, grad_scale, coef, decoupled, decay_factor);
                else adam_element(P[e], G[e], M[e], V[e], step_size, b1, b2, eps, wd, bc2_sqrt, grad_scale);
                if (AMAX && i + e >= amax_lo && i + e < amax_hi) mx = fmaxf(mx, fabsf(P[e]));
            }
            *reinterpret_cast<float4*>(p + i) = pp;
            *reinterpret_cast<float4*>(m + i) = mm;
            *reinterpret_cast<float4*>(v + i) = vv;
            if (zero_grad) *reinterpret_cast<float4*>(g + i) = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            for (long j = i; j < n; ++j) {
                if (EXT) adamw_element(p[j], g[j], m[j], v[j], step_size, b1, b2, eps, wd, bc2_sqrt, grad_scale, coef, decoupled, decay_factor);
                else adam_element(p[j], g[j], m[j], v[j], step_size, b1, b2, eps, wd, bc2_sqrt, grad_scale);
                if (AMAX && j >= amax_lo && j < amax_hi) mx = fmaxf(mx, fabsf(p[j]));
                if (zero_grad) g[j] = 0.f;
            }
        }
    }
    if (AMAX) {
        __shared__ float sh[4];
        mx = wave_max(mx);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mx;
        __syncthreads();
        if (threadIdx.x == 0) amax_part[blockIdx.x] = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
    }
}
