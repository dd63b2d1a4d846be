/* t4r_hip_rowclip.h -- global-norm gradient clipping ACROSS dense buckets and row-sparse tables: the row-sparse ("lazy") Adam
 * step of t4r_hip_rowadam.h cut in two, so that a table's gradient can enter the global norm of t4r_hip_optim.h before the
 * coefficient exists and be stepped with the coefficient after it.  The conventions are t4r_hip.h's (device pointers unless
 * marked "host", float = fp32, long = int64, `stream` a hipStream_t, nothing synchronises, nothing is allocated or copied,
 * argument errors -- checked before any launch -- come back negative with t4r_last_error() for the message, no state kept
 * between calls: what lives between the two halves lives in the CALLER's workspace).
 * Reference paths are relative to the reference repository root (NVIDIA-Merlin/Transformers4Rec).
 *
 * The reference trains through transformers4rec/torch/trainer.py (Trainer, a transformers.Trainer): AdamW with max_grad_norm =
 * 1.0, torch.nn.utils.clip_grad_norm_ over ALL parameters on every step, the embedding tables' dense [V, D] gradients among
 * them.  A table stepped lazily has no dense gradient; its non-zero rows are the compact [U, D] buffer the lazy step builds
 * anyway (U distinct rows, fp32 sums bit-identical to the dense scatter's), and every other row adds 0 to the norm.  The recipe:
 *
 *     for each dense bucket b:  n_b = t4r_grad_sumsq(stream, grad_b, numel_b, part + sum of the earlier counts)     (t4r_hip_optim.h)
 *     for each table t:         t4r_sort_ids(stream, ids_t, n_t, V_t, padding_idx, keys_t, perm_t, ...)             (t4r_hip.h)
 *                               n_t' = t4r_row_adam_reduce(stream, V_t, D_t, keys_t, perm_t, rows_t, ld, n_t, ws_t, bytes_t,
 *                                                          part + sum of the earlier counts)
 *     t4r_grad_clip_coef(stream, part, sum of all counts, grad_scale, max_norm, out2)                               (t4r_hip_optim.h)
 *     for each dense bucket b:  t4r_adamw_step(..., clip_coef = out2 + 1, ...)
 *     for each table t:         t4r_row_adam_apply(stream, param_t, exp_avg_t, exp_avg_sq_t, V_t, D_t, n_t, step, ...,
 *                                                  clip_coef = out2 + 1, ws_t, bytes_t)
 *
 * Neither U nor the coefficient visits the host.  No float atomics: the partials, and so the coefficient, are the same bits from
 * run to run and on every data-parallel rank that holds the same (ids, rows) and the same dense gradients.
 */
#ifndef T4R_HIP_ROWCLIP_H
#define T4R_HIP_ROWCLIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* The number of double partials t4r_row_adam_reduce writes for n lookups of width D: t4r_grad_sumsq_parts(n * D)
 * (t4r_hip_optim.h) -- a pure function of (n, D), non-decreasing in n, at most 2048; 0 for n <= 0 or D < 1.  It does not depend
 * on how many of the n lookups are distinct or valid: the host never learns that.  No launch. */
long t4r_row_grad_sumsq_parts(long n, int D);
/* replaces: a table's share of the per-parameter torch.linalg.vector_norm calls of torch.nn.utils.clip_grad_norm_
 * (transformers.Trainer's max_grad_norm step under transformers4rec/torch/trainer.py), taken over the dense [V, D] gradient the
 * reference's nn.Embedding produces -- here over its non-zero rows only.
 * keys, perm [n] int32: the outputs of t4r_sort_ids(ids, n, V, padding_idx); grad_rows [n, D] fp32 with row pitch ld_grad >= D
 * (elements), read only: all as for t4r_row_adam_step (t4r_hip_rowadam.h), whose first two stages these are, launch for launch --
 * the distinct valid keys are numbered 0 .. U-1 in key order and row u of a compact [U, D] buffer inside ws gets the sum of
 * grad_rows[perm[j]] over the run of key u, in the order and with the bits of t4r_embedding_bwd_sorted.  Then ONE more launch:
 *     part[b] = the sum over the elements workgroup b read of (double)g^2, g running over the first U * D floats of the compact
 *               buffer, for b < the returned count = t4r_row_grad_sumsq_parts(n, D).
 * The grid is sized from (n, D) and U is read on the device; a workgroup whose elements all lie past U * D stores 0.0, so
 * exactly that many slots are written whatever U is (U = 0 included) and later slots of part are not touched.  Every square and
 * every add is in double, thread, then wave, then workgroup, in t4r_grad_sumsq's fixed order.  Padding and out-of-range lookups
 * contribute nothing.  part is 8-byte aligned.
 * ws: at least t4r_row_adam_ws_bytes(n, D) bytes (t4r_hip_rowadam.h), 16-byte aligned, contents undefined before; AFTER the call
 * they are defined and belong to t4r_row_adam_apply with the same (n, D): keep the bytes, at the same address, unwritten, until
 * that call's launch has run (stream order is enough).  Nothing outside ws and the returned count of part is written.
 * n = 0: nothing launches, returns 0.  n, V < 2^31 - 1.  Returns the count, < 0 on an error. */
int t4r_row_adam_reduce(void* stream, long V, int D, const int* keys, const int* perm, const float* grad_rows, long ld_grad,
                        long n, void* ws, long ws_bytes, double* part);
/* replaces: torch.optim.AdamW.step / torch.optim.Adam.step after clip_grad_norm_ (transformers.Trainer's optimizer step under
 * transformers4rec/torch/trainer.py), restricted to the rows of an embedding table that have a gradient in this step.
 * The third stage of t4r_row_adam_step over the workspace a t4r_row_adam_reduce call with the same (n, D) left at ws: for every
 * distinct valid key r of that call, row r of param, exp_avg, exp_avg_sq [V, D] fp32 gets t4r_adamw_step's update
 * (t4r_hip_optim.h: same arithmetic) with the gradient (g * grad_scale) * coef -- two roundings, average first, then clip --,
 * g being the row's sum in the compact buffer and
 *   clip_coef   null, or a device pointer to ONE float (4-byte aligned; t4r_grad_clip_coef's out2 + 1), read once per thread.
 *               Null or a coefficient of exactly 1.0: the bits of t4r_row_adam_step over the same (keys, perm, grad_rows).
 * weight_decay, decoupled, step (the GLOBAL step, >= 1) and the 16-byte / scalar access rule are t4r_row_adam_step's.  Every
 * other row, and every byte outside the three [V, D] buffers, is neither read nor written; ws is only read, and undefined for the
 * caller afterwards.  V and D must be the reduce call's.  n = 0: nothing launches, returns 0.  0 on success. */
int t4r_row_adam_apply(void* stream, float* param, float* exp_avg, float* exp_avg_sq, long V, int D, long n, int step, float lr,
                       float beta1, float beta2, float eps, float weight_decay, int decoupled, float grad_scale,
                       const float* clip_coef, void* ws, long ws_bytes);

#ifdef __cplusplus
}
#endif
#endif /* T4R_HIP_ROWCLIP_H */
