/* t4r_hip_optim.h -- the optimizer entries of libt4r_hip.so beyond t4r_adam_step / t4r_adam_step_amax of t4r_hip.h: the global
 * gradient norm over flat gradient buffers, its clip coefficient, and the fused Adam step with that coefficient and with
 * decoupled weight decay (AdamW).  The conventions are t4r_hip.h's (device pointers unless marked "host", float = fp32, long =
 * int64, `stream` a hipStream_t, nothing synchronises, nothing is allocated or copied, argument errors -- checked before any
 * launch -- come back negative with t4r_last_error() for the message, no state kept between calls).
 * Reference paths are relative to the reference repository root (NVIDIA-Merlin/Transformers4Rec).
 *
 * The reference trains its paper configurations through transformers4rec/torch/trainer.py (Trainer, a transformers.Trainer): AdamW,
 * max_grad_norm = 1.0 -- torch.nn.utils.clip_grad_norm_ over all parameters on every step --, and a warm-up schedule
 * (trainer.py:243-313).  Here the parameters live in flat buckets, so the recipe is three kinds of launch:
 *
 *     for each bucket b:  n_b = t4r_grad_sumsq(stream, grad_b, numel_b, part + sum of the earlier n)
 *     t4r_grad_clip_coef(stream, part, sum of n_b, grad_scale, max_norm, out2)
 *     for each bucket b:  t4r_adamw_step(..., clip_coef = out2 + 1, ...)
 *
 * The coefficient never visits the host.  No float atomics: the norm is the same bits from run to run, and the same on every
 * data-parallel rank once the gradients are (after the all-reduce).
 * Non-finite gradients are not special-cased; they propagate as through clip_grad_norm_ (error_if_nonfinite=False): an infinite
 * norm gives a coefficient of 0 (and 0 * inf = NaN in the elements that were infinite), a NaN norm a NaN coefficient and so
 * NaN everywhere.
 */
#ifndef T4R_HIP_OPTIM_H
#define T4R_HIP_OPTIM_H

#ifdef __cplusplus
extern "C" {
#endif

/* The number of partial sums one t4r_grad_sumsq launch over n elements writes: min(max(ceil(floor(n / 4) / 256), 1), 2048) -- a
 * pure function of n, non-decreasing, at most 2048; 0 for n <= 0.  No launch. */
long t4r_grad_sumsq_parts(long n);
/* replaces: the per-parameter torch.linalg.vector_norm calls of torch.nn.utils.clip_grad_norm_ (transformers.Trainer's
 * max_grad_norm step under transformers4rec/torch/trainer.py).
 * grad [n] fp32, 16-byte aligned, read only.  part[b] = the sum over the elements workgroup b read of (double)grad[i]^2, for
 * b < the returned count = t4r_grad_sumsq_parts(n); later slots of part are not touched.  Every square and every add is in
 * double (a float squared is exact in double): thread, then wave, then workgroup, in a fixed order.  part is 8-byte aligned.
 * Returns the count (0 for n <= 0: nothing launches), < 0 on an error. */
int t4r_grad_sumsq(void* stream, const float* grad, long n, double* part);
/* replaces: the norm of norms, `clip_coef = max_norm / (total_norm + 1e-6)` and its clamp in torch.nn.utils.clip_grad_norm_
 * (the same max_grad_norm step under transformers4rec/torch/trainer.py).
 * One workgroup.  sum = the n_part partials (of all buckets, concatenated) added in double in an order fixed by n_part alone;
 *     out2[0] = norm = (float)(|grad_scale| * sqrt(sum))                  rounded once: the norm of the SCALED gradient
 *     out2[1] = coef = min(max_norm / (norm + 1e-6f), 1.0f)               in fp32; a NaN quotient stays NaN (torch.clamp)
 * max_norm > 0 (+inf: the coefficient is 1 whatever the norm, unless that is infinite too); n_part >= 1; out2 4-byte aligned.
 * 0 on success. */
int t4r_grad_clip_coef(void* stream, const double* part, int n_part, float grad_scale, float max_norm, float* out2);
/* replaces: torch.optim.AdamW.step / torch.optim.Adam.step after clip_grad_norm_ (transformers.Trainer's optimizer step under
 * transformers4rec/torch/trainer.py), one launch per flat buffer.
 * t4r_adam_step's update (t4r_hip.h: same arguments, same arithmetic, same grid) with
 *   clip_coef   null, or a device pointer to ONE float: the gradient the step sees is (grad * grad_scale) * coef -- two
 *               roundings, average first, then clip.  Null or a coefficient of exactly 1.0: the bits of t4r_adam_step.
 *   decoupled   0: weight_decay enters the gradient (g + weight_decay * p), torch.optim.Adam.  Non-zero: param is first
 *               multiplied by (float)(1.0 - (double)lr * (double)weight_decay), then updated without that term -- torch.optim.AdamW.
 *   amax_part   null, or as in t4r_adam_step_amax: amax_part[b] = max |param[i]| AFTER the update over i in [amax_lo, amax_hi)
 *               seen by workgroup b, 0 <= amax_lo < amax_hi <= n (the range is ignored when amax_part is null).
 * step >= 1; param, grad, exp_avg, exp_avg_sq 16-byte aligned.
 * Returns the number of workgroups (<= 512 with amax_part: the capacity it must have; <= 4096 without; 0 for n <= 0),
 * < 0 on an error. */
int t4r_adamw_step(void* stream, float* param, float* grad, float* exp_avg, float* exp_avg_sq, long n, int step,
                   float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled, float grad_scale,
                   int zero_grad, const float* clip_coef, long amax_lo, long amax_hi, float* amax_part);

#ifdef __cplusplus
}
#endif
#endif /* T4R_HIP_OPTIM_H */
