/* t4r_hip_rowadam.h -- the row-sparse ("lazy") Adam step of libt4r_hip.so for embedding tables: only the rows that have a
 * gradient in this step are read and written.  The conventions are t4r_hip.h's (device pointers unless marked "host", float =
 * fp32, long = int64, `stream` a hipStream_t, nothing synchronises, nothing is allocated or copied, argument errors -- checked
 * before any launch -- come back negative with t4r_last_error() for the message, no state kept between calls).
 * Reference paths are relative to the reference repository root (NVIDIA-Merlin/Transformers4Rec).
 *
 * The reference trains with torch.optim.Adam over dense gradients (Model.fit, transformers4rec/torch/model/base.py:669-718); its
 * nn.Embedding tables produce a dense [V, D] gradient and the optimizer streams every row.  Here the backward already leaves a
 * table's gradient as (ids, rows) -- the lookup scatter of the input block, the sampled-softmax head -- and the recipe is
 *
 *     t4r_sort_ids(stream, ids, n, V, padding_idx, keys, perm, ws_sort, ...)                      (t4r_hip.h)
 *     t4r_row_adam_step(stream, param, exp_avg, exp_avg_sq, V, D, keys, perm, rows, D, n, step, ..., ws, ws_bytes)
 *
 * No float atomics: the same bits from run to run, and on every data-parallel rank that holds the same (ids, rows).
 * The semantics are torch.optim.SparseAdam's: a row without a gradient keeps its parameters AND its moments (they do not decay),
 * while the bias corrections use the global step.  A dense Adam step moves such a row by its decaying first moment; the two
 * agree exactly only while the untouched rows' moments are zero.
 */
#ifndef T4R_HIP_ROWADAM_H
#define T4R_HIP_ROWADAM_H

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace t4r_row_adam_step needs for n lookups of width D: the rank arrays, the scan's scratch, a compact [n, D]
 * gradient buffer and the partial sums of the segmented sum.  A pure function of (n, D), non-decreasing in n; 0 for n <= 0 or
 * D < 1.  No launch. */
long t4r_row_adam_ws_bytes(long n, int D);
/* replaces: torch.optim.Adam.step of Model.fit (transformers4rec/torch/model/base.py:669-718), restricted to the rows that
 * have a gradient; with decoupled != 0 torch.optim.AdamW.step (transformers4rec/torch/trainer.py), restricted likewise.
 * param, exp_avg, exp_avg_sq [V, D] fp32, contiguous.  keys, perm [n] int32: the outputs of t4r_sort_ids(ids, n, V,
 * padding_idx) -- keys ascending, equal keys in lookup order, padding / out-of-range lookups with key V last.  grad_rows
 * [n, D] fp32 with row pitch ld_grad >= D (elements): row i is the gradient of lookup i; read only.
 * For every distinct key r < V:
 *     g     = the sum of grad_rows[perm[j]] over the run of r, in the order -- and so with the bits -- in which
 *             t4r_embedding_bwd_sorted adds the same (keys, perm, rows) into a zeroed [V, D] buffer;
 *     row r of param, exp_avg, exp_avg_sq gets t4r_adamw_step's update (t4r_hip_optim.h: same arithmetic, clip coefficient
 *             1) with the gradient g * grad_scale: weight_decay enters the gradient (decoupled = 0) or multiplies the row by
 *             (float)(1.0 - (double)lr * (double)weight_decay) first (decoupled != 0) -- for these rows only.
 * Every other row, and every byte outside the three [V, D] buffers and ws, is neither read nor written.  The bias corrections
 * 1 - beta1^step and sqrt(1 - beta2^step) are computed in double on the host from the GLOBAL step (>= 1).
 * Any D >= 1: 16-byte accesses when D % 4 == 0 and the three buffers are 16-byte aligned, scalar ones otherwise (4-byte
 * alignment is required).  ws: at least t4r_row_adam_ws_bytes(n, D) bytes, 16-byte aligned, contents undefined before and
 * after.  The number of distinct rows stays on the device: the grids are sized from n, surplus workgroups exit.
 * n = 0: nothing launches, returns 0.  n, V < 2^31 - 1.  0 on success. */
int t4r_row_adam_step(void* stream, float* param, float* exp_avg, float* exp_avg_sq, long V, int D, const int* keys,
                      const int* perm, const float* grad_rows, long ld_grad, long n, int step, float lr, float beta1,
                      float beta2, float eps, float weight_decay, int decoupled, float grad_scale, void* ws, long ws_bytes);

#ifdef __cplusplus
}
#endif
#endif /* T4R_HIP_ROWADAM_H */
