/* t4r_hip_gru.h -- the GRU body of libt4r_hip.so: a stack of 1 .. 4 GRU layers over a session, the whole time loop of a layer
 * in ONE launch with the recurrent weights resident in registers.  The conventions are t4r_hip.h's (device pointers, float =
 * fp32, long = int64, `stream` a hipStream_t, nothing synchronises, nothing is allocated or copied, argument errors -- checked
 * before any launch -- come back negative with t4r_last_error() for the message, no state kept between calls).  A feature
 * header: bound through _lib.FEATURE_HEADERS.
 * Reference paths are relative to the reference repository root (NVIDIA-Merlin/Transformers4Rec).
 *
 * The reference's session-based tutorial wraps torch.nn.GRU in a Block (transformers4rec/torch/block/base.py:87-106) and uses
 * it as the sequence model between the MLPBlock and the prediction task.
 *
 * Symbols: B sessions of L positions, T = B L token rows (b, t) at row b L + t (batch_first), n layers, H the hidden width,
 * layer k has W_ih [3H, K_k], W_hh [3H, H], b_ih [3H], b_hh [3H] in torch.nn.GRU's layout (gate order r | z | n), K_0 the
 * input width, K_k = H above.  Per session, t ascending, with h_{-1} = h0[k][b] (h0 NULL: zeros) and a_t the layer's input:
 *     gi_t = b_ih + W_ih a_t          gh_t = b_hh + W_hh h_{t-1}      fp32 fused multiply-adds on the matrix cores, seeded with
 *                                                                     the bias; K + 2 roundings bound either, in any order
 *     r = sig(gi_r + gh_r)    z = sig(gi_z + gh_z)    n = th(gi_n + r * gh_n)      (b_hn is INSIDE the reset product)
 *     h_t = n + z * (h_{t-1} - n)
 *     sig(v) = 1 / (1 + expf(-v))     th(v) = 1 - 2 / (1 + expf(2 v))       expf the device library's (<= 3 ulp), / the
 *                                                                            correctly rounded fp32 division, + and - fp32
 * Between layers (not after the last): a^{k+1}_t = drop_p > 0 ? h^k_t * m : h^k_t, m = keep(seed, ctr_hi_k, (b L + t) H + d) ?
 * fl(1 / (1 - drop_p)) : 0; keep is t4r_hip.h's dropout rule (the comment above t4r_dropout), ctr_hi_k =
 * t4r_dropout_ctr_hi(offset, layer = k, site = 9 (T4R_SITE_GRU)).  The recurrence carries the undropped h.
 * All L positions are computed.  The bits of a session's outputs do not depend on B nor on where the session sits in the batch.
 *
 * Host arrays: W_ih, W_hh, b_ih, b_hh, d_W_ih, d_W_hh, d_b_ih, d_b_hh (n device pointers each) are read on the host during the
 * call and not kept.
 *
 * Limits: 1 <= n <= 4, 1 <= K0 <= 1024, 1 <= H <= 128, 1 <= L <= 1023, B >= 0 with B L max(K0, 3H) < 2^31, 0 <= drop_p < 1.
 * Every pointer is 4-byte aligned; 16-byte requests are used for a row-major operand whose width is a multiple of 4 and whose
 * base is 16-byte aligned, single elements otherwise (the same bits either way).
 *
 * Launches: forward 2 per layer (the input product of all tokens, the recurrence), 2n in all, none of them per time step.
 * Backward 4 per layer (the time-reversed recurrence, the product for the layer's d input, the partial products of
 * [d W_ih | d b_ih] and [d W_hh | d b_hh], their sums), at most 4n in all.
 */
#ifndef T4R_HIP_GRU_H
#define T4R_HIP_GRU_H

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when (n, K0, H, L) is within the limits above, else 0.  No launch. */
int t4r_gru_supported(int n, int K0, int H, int L);
/* Floats of the forward's `saved` buffer (training form): per layer the gate values r, z, n and gh_n of every token, and for
 * the layers below the last their outputs h and a.  A pure function of its arguments, non-decreasing in B; 0 for B <= 0 and
 * for anything outside the limits.  No launch. */
long t4r_gru_saved_floats(long B, int L, int n, int K0, int H);
/* Floats of workspace t4r_gru_fwd needs (gi of one layer; in the inference form also the lower layers' outputs).  As above. */
long t4r_gru_fwd_ws_floats(long B, int L, int n, int K0, int H);
/* Floats of workspace t4r_gru_bwd needs (the pre-activation gradients of one layer, the gradient handed to the layer below,
 * the per-split partials of the weight gradients).  As above. */
long t4r_gru_bwd_ws_floats(long B, int L, int n, int K0, int H);
/* replaces: torch.nn.GRU(batch_first=True).forward as wrapped by Block (transformers4rec/torch/block/base.py:87-106), its
 * output tensor only.
 * x [B, L, K0] dense.  h0: NULL or [n, B, H].  b_ih, b_hh: NULL, or n pointers of which any may be NULL (no such bias).
 * out [B, L, H]: the last layer's h.  saved: NULL (inference form: only out is written) or t4r_gru_saved_floats(...) floats
 * (training form: filled for t4r_gru_bwd; its layout is the kernels' business).  ws: t4r_gru_fwd_ws_floats(...) floats,
 * contents undefined before and after.
 * 2n launches.  B = 0: nothing launches, returns 0.  0 on success. */
int t4r_gru_fwd(void* stream, const float* x, const float* h0, const float* const* W_ih, const float* const* W_hh,
                const float* const* b_ih, const float* const* b_hh, float* out, float* saved, float* ws, long B, int L, int n,
                int K0, int H, float drop_p, unsigned long long seed, unsigned long long offset);
/* replaces: the autograd backward of torch.nn.GRU(batch_first=True) as wrapped by Block
 * (transformers4rec/torch/block/base.py:87-106) with respect to its input and its parameters.
 * dout [B, L, H] read only; x, h0, W_ih, W_hh, out, saved, drop_p, seed, offset as given to / written by the forward.  With
 * dh_t = dout_t (for a lower layer: the upper layer's d input times its mask) + the carry from step t + 1:
 *     dn = dh (1 - z)   dpre_n = dn (1 - n n)   dpre_z = dh (h_{t-1} - n) z (1 - z)   dpre_r = dpre_n gh_n r (1 - r)
 *     dgi = [dpre_r | dpre_z | dpre_n]   dgh = [dpre_r | dpre_z | dpre_n r]   carry_{t-1} = dh z + W_hh^T dgh
 *     d_W_ih += sum dgi a^T   d_b_ih += sum dgi   d_W_hh += sum dgh h_{t-1}^T   d_b_hh += sum dgh   d a = W_ih^T dgi
 * dx [B, L, K0] is overwritten; d_W_ih[k], d_W_hh[k], d_b_ih[k], d_b_hh[k] are ACCUMULATED.  dx, the four arrays and each of
 * their entries may be NULL.  x is read for d_W_ih[0] and d_b_ih[0] only (else it may be NULL).  The batch sums go through
 * per-split partials in ws, tokens ascending within a split, added in split order: no float atomics, the same bits from run to
 * run.  ws: t4r_gru_bwd_ws_floats(...) floats, contents undefined before and after.
 * At most 4n launches.  B = 0: nothing launches, returns 0.  0 on success. */
int t4r_gru_bwd(void* stream, const float* dout, const float* x, const float* h0, const float* const* W_ih,
                const float* const* W_hh, const float* out, const float* saved, float* dx, float* const* d_W_ih,
                float* const* d_W_hh, float* const* d_b_ih, float* const* d_b_hh, float* ws, long B, int L, int n, int K0, int H,
                float drop_p, unsigned long long seed, unsigned long long offset);

#ifdef __cplusplus
}
#endif
#endif /* T4R_HIP_GRU_H */
