/* t4r_hip_sampling.h -- the sampling entries of libt4r_hip.so: Gumbel noise over item scores, and the two fused top-k heads
 * of t4r_hip.h as SAMPLERS.  The conventions are t4r_hip.h's (device pointers unless marked "host", dense row-major, float =
 * fp32, long = int64, `stream` a hipStream_t, nothing synchronises unless said, 0 on success, -1 on an argument error -- checked
 * before any launch --, a hipError_t value on a launch error, t4r_last_error() for the message, no state kept between calls).
 * Reference paths are relative to the reference repository root (NVIDIA-Merlin/Transformers4Rec).
 *
 * The noise.  One draw is a pure function of (seed, ctr_hi, row, item) and of nothing else -- not of n_rows, V, a pitch, a tile
 * or the entry that asks for it:
 *     block = Philox4x32-10(key = seed, counter words c0 = item, c1 = row >> 2, (c2, c3) = ctr_hi)
 *     w     = word (row & 3) of the block
 *     u     = ((w >> 9) + 0.5) * 2^-23            exact in fp32, in [2^-24, 1 - 2^-24]
 *     g     = -log(-log u)                         in [-2.81, 16.64]
 * and a perturbed score is fp32(s + g): one add, one rounding.  `row` = row0 + the row's index in the call, so a caller that
 * splits its rows over several calls (or ranks) draws what one call would have drawn.  ctr_hi is the caller's stream position;
 * the Python side uses t4r_dropout_ctr_hi(offset, 255, 7) (site 7 = SITE_GUMBEL).  A call is replayable from (seed, ctr_hi, row0).
 *
 * argmax over items of (s + g) is a draw from softmax(s); the k largest are k draws without replacement in proportion to
 * softmax(s) (Gumbel top-k).  This is the distribution of the reference's draw, not its bits: the reference takes torch.rand and
 * adds 1e-9 twice (transformers4rec/torch/masking.py:866-867).
 */
#ifndef T4R_HIP_SAMPLING_H
#define T4R_HIP_SAMPLING_H

#ifdef __cplusplus
extern "C" {
#endif

/* replaces: transformers4rec/torch/masking.py:866-868 (sample_from_softmax: torch.rand, two logs, logits + gumbel_noise).
 * In place on scores [n_rows, >= V] fp32 with row pitch ld >= V: scores[r, c] = fp32(scores[r, c] + g(row0 + r, c * item_stride)).
 * Column c stands for item c * item_stride (item_stride >= 1; 1: the columns are the items).  Columns V .. ld - 1 are not
 * touched.  row0 >= 0. */
int t4r_gumbel_add_f32(void* stream, float* scores, int n_rows, int V, long ld, long row0, int item_stride,
                       unsigned long long seed, unsigned long long ctr_hi);
/* replaces: transformers4rec/torch/masking.py:866-870 (sample_from_softmax whole: noise, add, softmax, argmax over [N_m, V]).
 * One pass over scores [n_rows, >= V] (read only, row pitch ld >= V), no perturbed copy: out_val[r] = max over c of
 * fp32(scores[r, c] + g(row0 + r, c)), out_idx[r] = its c, ties to the lower c -- bit for bit t4r_topk(k = 1) of what
 * t4r_gumbel_add_f32 (item_stride 1) leaves. */
int t4r_gumbel_argmax_f32(void* stream, const float* scores, int n_rows, int V, long ld, long row0, unsigned long long seed,
                          unsigned long long ctr_hi, float* out_val, long* out_idx);
/* replaces: model/prediction_task.py:664 (the scores alpha * X @ W^T) + masking.py:866-870 on them, and for k > 1 the
 * score-proportional draw of k distinct items a stochastic recommender takes from those scores, where the [n_rows, V] scores
 * should not exist.  t4r_item_topk_f32 / t4r_item_topk_h16 (t4r_hip.h: arguments, k, outputs, workspace rules, host_stats,
 * the one synchronisation of `stream`) over the perturbed score fp32(s[r, v] + g(row0 + r, v)), s = the bits of the materialised
 * scores (t4r_gemm_f32 in precision mode 0 / t4r_item_scores_h16): out_val [n_rows, k] the perturbed scores, descending, out_idx
 * their items, ties to the lower index -- bit for bit t4r_topk(k) of t4r_gumbel_add_f32 over those scores, for every input.
 * 1 <= k <= min(256, V); ldx, ldw >= D; the image as t4r_item_topk_h16 takes it.
 * workspace: t4r_item_sample_ws_bytes / t4r_item_sample_h16_ws_bytes(n_rows, V, D, k) bytes, 16-byte aligned. */
long t4r_item_sample_ws_bytes(int n_rows, int V, int D, int k);
int t4r_item_sample_f32(void* stream, int n_rows, int V, int D, float alpha, const float* X, long ldx, const float* W,
                        long ldw, int k, float* out_val, long* out_idx, void* workspace, long ws_bytes, long* host_stats,
                        long row0, unsigned long long seed, unsigned long long ctr_hi);
long t4r_item_sample_h16_ws_bytes(int n_rows, int V, int D, int k);
int t4r_item_sample_h16(void* stream, int n_rows, int V, int D, float alpha, const float* X, long ldx, const void* image,
                        long ldp, int dtype, int k, float* out_val, long* out_idx, void* workspace, long ws_bytes,
                        long* host_stats, long row0, unsigned long long seed, unsigned long long ctr_hi);

#ifdef __cplusplus
}
#endif
#endif /* T4R_HIP_SAMPLING_H */
