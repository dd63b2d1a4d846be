/* t4r_hip_filter.h -- the item-filter entries of libt4r_hip.so: which items the two fused top-k heads of t4r_hip.h and their
 * sampling forms of t4r_hip_sampling.h may return, and the same filter over materialised scores.  The conventions are
 * t4r_hip.h's (device pointers unless marked "host", dense row-major, float = fp32, long = int64, `stream` a hipStream_t,
 * nothing synchronises unless said, 0 on success, -1 on an argument error -- checked before any launch --, a hipError_t value on
 * a launch error, t4r_last_error() for the message, no state kept between calls).
 * Reference paths are relative to the reference repository root (NVIDIA-Merlin/Transformers4Rec).
 *
 * The reference has no such option: its inference hands the caller the full [N, V] scores
 * (transformers4rec/torch/model/prediction_task.py:452-470) and the caller writes `scores[mask] = -inf` before torch.topk.  The
 * fused heads never write those scores, so the filter is an argument.
 *
 * The filter.  Two optional parts, one definition for every entry below:
 *   allow_bits   a catalogue filter shared by all rows: a bit array over the items, bit (v & 31) of 32-bit word (v >> 5) set
 *                where item v may be returned.  t4r_item_allow_words(V) = 2 * ceil(V / 64) words, 4-byte aligned; bits at and
 *                beyond V are zero (t4r_item_allow_pack writes them so).  Null: every item is allowed.
 *   excl         a per-row exclusion list (the items a session has seen): [n_rows, n_excl] int64 with row pitch
 *                ld_excl >= n_excl, 0 <= n_excl <= 1024, every row in non-decreasing order.  Entries outside [0, V) are ignored
 *                (-1 pads), duplicates are fine.  Null or n_excl = 0: no list.  Rows that are NOT sorted are memory-safe; for
 *                them it is unspecified which of the listed items are excluded.
 *   allowed(row, v) = (allow_bits null or bit v set) and v not in the row's list.
 *   The filtered score of (row, v) is the score where allowed(row, v), -inf otherwise.
 * Both buffers are the caller's and read-only; the workspaces do not grow.
 *
 * The tail rule.  A row with fewer than k allowed items whose score is above -inf ends in slots of value -inf: every output
 * slot whose value is -inf has id -1.
 */
#ifndef T4R_HIP_FILTER_H
#define T4R_HIP_FILTER_H

#ifdef __cplusplus
extern "C" {
#endif

/* words of an allow_bits array over V items: 2 * ceil(V / 64); 0 for V <= 0.  No launch. */
long t4r_item_allow_words(int V);
/* replaces: the boolean mask tensor of `scores[:, ~allow] = -inf` on the scores of model/prediction_task.py:452-470.
 * allow [V] bytes (non-zero = allowed) -> bits [t4r_item_allow_words(V)], pad bits zero. */
int t4r_item_allow_pack(void* stream, const unsigned char* allow, int V, unsigned* bits);
/* replaces: `scores[mask] = -inf` on the scores of model/prediction_task.py:452-470, before torch.topk.
 * In place on scores [n_rows, >= V] fp32 with row pitch ld >= V: column c stands for item c * item_stride (item_stride >= 1;
 * 1: the columns are the items, as t4r_gumbel_add_f32 counts them) and becomes -inf where that item is not allowed, whatever it
 * held (NaN included).  Allowed columns and columns V .. ld - 1 are not touched; the scores are never read.  allow_bits covers
 * the items 0 .. (V - 1) * item_stride; excl row r belongs to scores row r. */
int t4r_item_mask_f32(void* stream, float* scores, int n_rows, int V, long ld, int item_stride, const unsigned* allow_bits,
                      const long* excl, int n_excl, long ld_excl);
/* replaces: `scores[mask] = -inf` + torch.topk on the scores of model/prediction_task.py:452-470 (:664), where the
 * [n_rows, V] scores should not exist.  t4r_item_topk_f32 / t4r_item_topk_h16 (t4r_hip.h: arguments, k, outputs, host_stats, the one
 * synchronisation of `stream`) over the filtered score: bit for bit t4r_topk(k) of t4r_item_mask_f32 over the materialised
 * scores, then the tail rule -- for every input.  An excluded item never enters a candidate list: a filter changes no workspace
 * size and overflows no list by itself.
 * workspace: that of the unfiltered entry, t4r_item_topk_ws_bytes / t4r_item_topk_h16_ws_bytes(n_rows, V, D, k). */
int t4r_item_topk_filtered_f32(void* stream, int n_rows, int V, int D, float alpha, const float* X, long ldx, const float* W,
                               long ldw, int k, float* out_val, long* out_idx, void* workspace, long ws_bytes, long* host_stats,
                               const unsigned* allow_bits, const long* excl, int n_excl, long ld_excl);
int t4r_item_topk_filtered_h16(void* stream, int n_rows, int V, int D, float alpha, const float* X, long ldx, const void* image,
                               long ldp, int dtype, int k, float* out_val, long* out_idx, void* workspace, long ws_bytes,
                               long* host_stats, const unsigned* allow_bits, const long* excl, int n_excl, long ld_excl);
/* replaces: the same `scores[mask] = -inf` on the scores of model/prediction_task.py:452-470 before a score-proportional draw
 * (masking.py:866-870 on them).  t4r_item_sample_f32 / t4r_item_sample_h16 (t4r_hip_sampling.h) over the filtered perturbed
 * score: bit for bit t4r_topk(k) of t4r_item_mask_f32 over t4r_gumbel_add_f32 over the materialised scores, then the tail rule:
 * k draws without replacement in proportion to the softmax over the ALLOWED items.  excl row r belongs to row r of the call
 * (stream row row0 + r).
 * workspace: t4r_item_sample_ws_bytes / t4r_item_sample_h16_ws_bytes(n_rows, V, D, k). */
int t4r_item_sample_filtered_f32(void* stream, int n_rows, int V, int D, float alpha, const float* X, long ldx, const float* W,
                                 long ldw, int k, float* out_val, long* out_idx, void* workspace, long ws_bytes,
                                 long* host_stats, long row0, unsigned long long seed, unsigned long long ctr_hi,
                                 const unsigned* allow_bits, const long* excl, int n_excl, long ld_excl);
int t4r_item_sample_filtered_h16(void* stream, int n_rows, int V, int D, float alpha, const float* X, long ldx,
                                 const void* image, long ldp, int dtype, int k, float* out_val, long* out_idx, void* workspace,
                                 long ws_bytes, long* host_stats, long row0, unsigned long long seed, unsigned long long ctr_hi,
                                 const unsigned* allow_bits, const long* excl, int n_excl, long ld_excl);

#ifdef __cplusplus
}
#endif
#endif /* T4R_HIP_FILTER_H */
