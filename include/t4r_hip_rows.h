/* t4r_hip_rows.h -- the row-mapped forms of the XLNet layer's row-wise kernels in libt4r_hip.so: the feed-forward block and
 * LayerNorm-1 backward on a SUBSET of the token rows.  The conventions are t4r_hip.h's (device pointers, float = fp32,
 * long = int64, `stream` a hipStream_t, nothing synchronises, nothing is allocated or copied, argument errors -- checked
 * before any launch -- come back non-zero with t4r_last_error() for the message, no state kept between calls).
 *
 * Why: the last layer of a stack whose consumer reads the output at the label rows only (the next-item head gathers them and
 * returns a gradient that is exactly zero everywhere else).  The feed-forward block and LayerNorm-1 are row-wise, so their
 * forward and backward on the other rows is work nobody reads.
 *
 * The map: rows [n] int32 on the device, ASCENDING, UNIQUE, every value in [0, T); 1 <= n <= T.  It travels in the launch
 * parameters.  Workgroup tile i works on compact rows [i 16 R, ...); everything that identifies a TOKEN -- the loads of the
 * [T, .] inputs, the stores of the [T, .] outputs, every Philox counter -- uses t = rows[compact], so a row's result is the
 * same bits whichever tile it sits in and whether or not a map is given.  Buffers that only feed the backward and the weight
 * gradients are in COMPACT order ([n, .]): the token-reducing products then run with K = n.
 *
 * The contract of the two layer entries: "zero off the map" out of the forward (h_out is zero at every row not in the map,
 * zeroed by the entry), "read only on the map" in the backward (dh_out is read ONLY at the mapped rows: the caller guarantees
 * that the gradient is zero elsewhere).  Per-row results equal the plain entries' bit for bit; the batch-reduced parameter
 * gradients equal them up to summation order.
 */
#ifndef T4R_HIP_ROWS_H
#define T4R_HIP_ROWS_H

#ifdef __cplusplus
extern "C" {
#endif

/* t4r_xlnet_ff_fwd (t4r_hip.h) on the mapped rows.  h1 [T, D] is read and hout [T, D], mean / rstd [T] are written at the
 * mapped rows only (the other rows of hout, mean, rstd are left as they are); ffpre / ffact [n, 4D] and ffout [n, D] are
 * written in compact order (all given, or all null with drop_p == 0). */
int t4r_xlnet_ff_fwd_rows(void* stream, const float* h1, const float* planes, const float* b1, const float* b2,
                          const float* gamma, const float* beta, float* ffpre, float* ffact, float* ffout, float* mean,
                          float* rstd, float* hout, int T, int D, float eps, float drop_p, unsigned long long seed,
                          unsigned long long ctr_act, unsigned long long ctr_out, const int* rows, int n);
/* t4r_xlnet_ff_bwd (t4r_hip.h) on the mapped rows.  dy, h1 [T, D], mean, rstd [T] are read at the mapped rows only; ffout
 * [n, D], ffpre [n, 4D] are what t4r_xlnet_ff_fwd_rows left; dh1, dffout [n, D], dpre [n, 4D] and h1_rows [n, D] (the mapped
 * rows of h1: the operand of d W1 += dpre^T @ h1_rows) are written in compact order.  part: as for T rows or for n. */
int t4r_xlnet_ff_bwd_rows(void* stream, const float* dy, const float* ffout, const float* h1, const float* mean,
                          const float* rstd, const float* gamma, const float* ffpre, const float* planes, float* dh1,
                          float* dffout, float* dpre, float* d_gamma, float* d_beta, float* d_b2, float* d_b1, float* part,
                          int T, int D, float drop_p, unsigned long long seed, unsigned long long ctr_act,
                          unsigned long long ctr_out, const int* rows, int n, float* h1_rows);
/* t4r_xlnet_ln1_bwd (t4r_hip.h) on the mapped rows.  dy [n, D] is in compact order (the dh1 of t4r_xlnet_ff_bwd_rows); ao,
 * h [T, D], mean, rstd [T] are read at the mapped rows only; dh, dao, dav [T, D] are ZEROED by this entry (on `stream`) and
 * written at the mapped rows.  part: as for T rows or for n. */
int t4r_xlnet_ln1_bwd_rows(void* stream, const float* dy, const float* ao, const float* h, const float* mean,
                           const float* rstd, const float* gamma, const float* planes, float* dh, float* dao, float* dav,
                           float* d_gamma, float* d_beta, float* part, long T, int D, float drop_p, unsigned long long seed,
                           unsigned long long ctr_hi, const int* rows, int n);

/* t4r_xlnet_layer_fwd (t4r_hip.h: same arguments, same workspace) with the feed-forward block on the mapped rows: the
 * attention half runs on all T = B L rows as ever, h_out is zero at every row not in the map.  The compact activations live
 * in the workspace slots of the full-size ones.  Refused (non-zero, before any launch): n < 1, n > T, null rows, key_len
 * given, a shape the token-tile kernels (d_model 32 / 64 / 128) and the one-kernel attention forward
 * (t4r_xlnet_attn_block_supported) do not take. */
int t4r_xlnet_layer_fwd_rows(void* stream, const float* h, const float* pos_emb, const float* const* params, float* ws,
                             float* h_out, int B, int L, int D, int n_head, float ln_eps, float drop_p,
                             unsigned long long seed, unsigned long long offset, int layer_idx, const int* key_len,
                             const float* pos_emb_b, const int* rows, int n);
/* t4r_xlnet_layer_bwd (t4r_hip.h: same arguments, bws of t4r_xlnet_layer_bwd_ws_floats) of a layer whose forward was
 * t4r_xlnet_layer_fwd_rows with the same map.  dh_out is read only at the mapped rows.  The feed-forward and LayerNorm-1
 * backward, the two feed-forward weight gradients and the column sums (d gamma, d beta, d b1, d b2) run over n rows; the
 * attention core's backward and d h run on all rows.  Same refusals as the forward. */
int t4r_xlnet_layer_bwd_rows(void* stream, const float* h, const float* pos_emb, const float* const* params,
                             float* const* grads, const float* ws, float* bws, const float* dh_out, float* dh_in, int B,
                             int L, int D, int n_head, float ln_eps, float drop_p, unsigned long long seed,
                             unsigned long long offset, int layer_idx, const int* key_len, const float* pos_emb_b,
                             const int* rows, int n);

#ifdef __cplusplus
}
#endif
#endif /* T4R_HIP_ROWS_H */
