// Global-norm gradient clipping and AdamW over flat buckets (C ABI: include/t4r_hip_optim.h).
//   t4r_grad_sumsq      : sum of squares of a flat gradient buffer, one double partial per workgroup (no atomics)
//   t4r_grad_clip_coef  : partials of all buckets -> norm and clip coefficient, on the device
//   t4r_adamw_step      : adam_kernel (adam_kernel.h) with the coefficient read from device memory and decoupled weight decay
// The reference's Trainer (transformers4rec/torch/trainer.py, a transformers.Trainer) runs clip_grad_norm_(max_grad_norm) and
// AdamW on every step; see the header for what each entry replaces.
#include "t4r_common.h"
#include "adam_kernel.h"
#include "sumsq_kernel.h"
#include <math.h>

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, long n, double* __restrict__ part) {
    const double acc = sumsq_block(g, n, sumsq_first(), sumsq_stride());
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// One workgroup: thread t adds partials t, t + 256, ... in index order, then the same wave / workgroup order as above.
// norm is rounded to fp32 once; the coefficient is torch.nn.utils.clip_grad_norm_'s fp32 arithmetic on it.  `c > 1 ? 1 : c`
// is torch.clamp(max=1): a NaN quotient (NaN or inf / inf) stays NaN.
__global__ __launch_bounds__(256) void grad_clip_coef_kernel(const double* __restrict__ part, int n_part, float grad_scale,
                                                             float max_norm, float* __restrict__ out2) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_part; i += 256) acc += part[i];
    acc = block_sum_d(acc);
    if (threadIdx.x == 0) {
        const float norm = (float)(fabs((double)grad_scale) * sqrt(acc));
        const float c = max_norm / (norm + 1e-6f);
        out2[0] = norm;
        out2[1] = c > 1.0f ? 1.0f : c;
    }
}

extern "C" long t4r_grad_sumsq_parts(long n) { return sumsq_parts(n); }

extern "C" int t4r_grad_sumsq(void* stream, const float* grad, long n, double* part) {
    if (n <= 0) return 0;
    T4R_CHECK_ARG(grad && part, "grad_sumsq: grad and part must not be null");
    T4R_CHECK_ARG((uintptr_t)grad % 16 == 0, "grad_sumsq: grad must be 16-byte aligned");
    T4R_CHECK_ARG((uintptr_t)part % 8 == 0, "grad_sumsq: part must be 8-byte aligned");
    const long blocks = t4r_grad_sumsq_parts(n);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, grad, n, part);
    if (hipGetLastError() != hipSuccess) { t4r_set_error("grad_sumsq: launch failed"); return -2; }
    return (int)blocks;
}

extern "C" int t4r_grad_clip_coef(void* stream, const double* part, int n_part, float grad_scale, float max_norm, float* out2) {
    T4R_CHECK_ARG(max_norm > 0.f, "grad_clip_coef: max_norm must be greater than 0");
    T4R_CHECK_ARG(n_part >= 1, "grad_clip_coef: n_part must be at least 1");
    T4R_CHECK_ARG(part && out2, "grad_clip_coef: part and out2 must not be null");
    T4R_CHECK_ARG((uintptr_t)part % 8 == 0 && (uintptr_t)out2 % 4 == 0, "grad_clip_coef: part must be 8-byte, out2 4-byte aligned");
    hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, n_part, grad_scale, max_norm, out2);
    T4R_LAUNCH_CHECK();
    return 0;
}

extern "C" int t4r_adamw_step(void* stream, float* param, float* grad, float* exp_avg, float* exp_avg_sq, long n, int step,
                              float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled, float grad_scale,
                              int zero_grad, const float* clip_coef, long amax_lo, long amax_hi, float* amax_part) {
    if (n <= 0) return 0;
    T4R_CHECK_ARG(step >= 1, "adamw: step is 1-based");
    T4R_CHECK_ARG(((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16 == 0,
                  "adamw: buffers must be 16-byte aligned");
    T4R_CHECK_ARG(param && grad && exp_avg && exp_avg_sq, "adamw: buffers must not be null");
    T4R_CHECK_ARG((uintptr_t)clip_coef % 4 == 0, "adamw: clip_coef must be 4-byte aligned");
    T4R_CHECK_ARG(!amax_part || (amax_lo >= 0 && amax_hi <= n && amax_lo < amax_hi), "adamw: the amax range must lie inside the buffer");
    // as t4r_adam_step: the bias corrections, and the decay factor with them, in double from the float arguments, rounded once
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    const float bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    const float factor = (float)(1.0 - (double)lr * (double)weight_decay);
    long blocks = (n / 4 + 255) / 256;
    const long cap = amax_part ? 512 : 4096;       // the grids of t4r_adam_step_amax / t4r_adam_step: their partials, their bits
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    if (amax_part)
        hipLaunchKernelGGL((adam_kernel<true, true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                           exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale, zero_grad, amax_lo, amax_hi,
                           amax_part, clip_coef, decoupled, factor);
    else
        hipLaunchKernelGGL((adam_kernel<false, true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                           exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale, zero_grad, 0L, 0L,
                           nullptr, clip_coef, decoupled, factor);
    if (hipGetLastError() != hipSuccess) { t4r_set_error("adamw: launch failed"); return -2; }
    return (int)blocks;
}
