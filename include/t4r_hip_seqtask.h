/* t4r_hip_seqtask.h -- the session-level prediction tasks of libt4r_hip.so: one label per session (binary classification,
 * regression) predicted from a summary of the body's output.  The conventions are t4r_hip.h's (device pointers, float = fp32,
 * long = int64, `stream` a hipStream_t, nothing synchronises, nothing is allocated or copied, argument errors -- checked
 * before any launch -- come back negative with t4r_last_error() for the message, no state kept between calls).
 * Reference paths are relative to the reference repository root (NVIDIA-Merlin/Transformers4Rec).
 *
 * The reference runs, per task, SequenceSummary(summary_type) over the body's [B, L, D] output, torch.nn.Linear(D, 1)
 * (with a bias for regression, without for binary classification), torch.nn.Sigmoid for the binary task, a squeeze and
 * torch.nn.BCELoss / torch.nn.MSELoss with the mean reduction (transformers4rec/torch/model/prediction_task.py:66-303,
 * model/base.py:84-232): about six small launches forward and eight backward.  Here each direction is two launches.
 *
 * With n_b = L where len is NULL, else min(max(len[b], 0), L):
 *     summary 0 (first)  s_b = x[b, 0, :]
 *     summary 1 (last)   s_b = x[b, n_b - 1, :]         (len NULL: position L - 1, padding included, as the reference)
 *     summary 2 (mean)   s_b = (sum_{l < n_b} x[b, l, :]) / n_b, one fp32 chain per (b, d), l ascending
 *     n_b = 0 (possible with len only): s_b = 0, and the session's dx rows are 0 in every mode
 *     z_b    = (b ? b[0] : 0) + sum_d w[d] s_b[d]
 *     pred_b = 1 / (1 + exp(-z_b)) for act 1, z_b for act 0
 *     row_b  = (pred_b - t_b)^2                                                         loss_kind 0 (MSE)
 *              -(t_b max(log p_b, -100) + (1 - t_b) max(log(1 - p_b), -100))            loss_kind 1 (BCE; needs act 1)
 *     loss   = (1 / B) sum_b row_b
 * Determinism: no float atomics, every sum in one fixed order, the same bits from run to run; s_b, pred_b and dx[b] are
 * the same bits wherever session b sits in the launch, whatever B is (dx through the one factor g / B) and whichever of
 * the 16-byte and 4-byte access paths runs.
 *
 * Limits: 1 <= L <= 1023 positions, 1 <= D <= 1024 columns, 0 <= B < 2^31 sessions.
 */
#ifndef T4R_HIP_SEQTASK_H
#define T4R_HIP_SEQTASK_H

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when (L, D) is within the limits above, else 0.  No launch. */
int t4r_seq_task_supported(int L, int D);
/* Floats of workspace t4r_seq_task_fwd and t4r_seq_task_bwd need for B sessions: B row values plus one [D + 1] partial per
 * chunk of sessions.  A pure function of its arguments, non-decreasing in B and D; 0 for B <= 0 or D outside the limits.
 * No launch. */
long t4r_seq_task_ws_floats(long B, int D);
/* replaces: SequenceSummary + torch.nn.Linear(D, 1) + torch.nn.Sigmoid + squeeze + torch.nn.BCELoss / torch.nn.MSELoss
 * (transformers4rec/torch/model/prediction_task.py:66-303: BinaryClassificationTask, RegressionTask;
 * model/base.py:84-232: PredictionTask.forward, compute_loss).
 * x [B, L, D] fp32 dense, the body's output.  len: int32 [B] or NULL.  w [D], b [1] or NULL.  target [B] fp32 or NULL.
 * s [B, D] and pred [B] are written (every element): caller-owned notes that t4r_seq_task_bwd reads.  With a target,
 * loss[0] is written and ws[0 .. B) holds the row losses afterwards; with target NULL (inference) loss and ws are not
 * touched and may be NULL.  16-byte accesses when D % 4 == 0 and x, w and s are 16-byte aligned, 4-byte ones otherwise
 * (4-byte alignment is required); the same bits either way.
 * ws: at least t4r_seq_task_ws_floats(B, D) floats.  Two launches (one for inference).
 * B = 0: nothing launches, returns 0.  0 on success. */
int t4r_seq_task_fwd(void* stream, const float* x, const int* len, long B, int L, int D, int summary, const float* w, const float* b,
                     int act, int loss_kind, const float* target, float* s, float* pred, float* loss, float* ws);
/* replaces: the autograd backward of the same chain (torch's mse_loss_backward / binary_cross_entropy_backward,
 * sigmoid_backward, the Linear's and the summary's backward; transformers4rec/torch/model/prediction_task.py:66-303).
 * g: device [1], the upstream gradient of loss.  pred, s: the forward's notes; target, len, w, summary, act, loss_kind as in
 * the forward.
 *     MSE:               dz_b = (g / B) 2 (pred_b - t_b)             (through p (1 - p) as well when act = 1)
 *     BCE over sigmoid:  dz_b = (g / B) (p_b - t_b) / max(p_b (1 - p_b), 1e-12) * p_b (1 - p_b)
 * so a saturated row (p exactly 0 or 1) has zero gradient, as in the reference.
 *     dx[b, l, :] = dz_b c_bl w      c_bl: first 1 at l = 0; last 1 at l = n_b - 1; mean 1 / n_b for l < n_b; else 0
 *     d_w[d] += sum_b dz_b s_b[d]    d_w [D], may be NULL
 *     d_b[0] += sum_b dz_b           d_b [1], may be NULL
 * dx [B, L, D] dense: EVERY element is written, the caller pre-fills nothing.  The sums are ACCUMULATED into d_w and d_b:
 * chunks of sessions are summed by one workgroup each in session order, their partials -- in ws -- in chunk order.
 * ws: at least t4r_seq_task_ws_floats(B, D) floats; ws[0 .. B) holds dz afterwards, the rest is undefined.
 * Two launches (one when d_w and d_b are both NULL).  B = 0: nothing launches, returns 0.  0 on success. */
int t4r_seq_task_bwd(void* stream, const float* g, const float* pred, const float* target, const float* s, const int* len, long B,
                     int L, int D, int summary, const float* w, int act, int loss_kind, float* dx, float* d_w, float* d_b, float* ws);

#ifdef __cplusplus
}
#endif
#endif /* T4R_HIP_SEQTASK_H */
