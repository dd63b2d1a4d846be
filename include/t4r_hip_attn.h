/* t4r_hip_attn.h -- the two XLNet attention entries of libt4r_hip.so that hand the attention probabilities from the forward
 * to the backward.  The conventions are t4r_hip.h's (device pointers, float = fp32, long = int64, `stream` a hipStream_t,
 * nothing synchronises, nothing is allocated or copied, argument errors -- checked before any launch -- come back non-zero
 * with t4r_last_error() for the message, no state kept between calls).
 *
 * prob [B][n_head][L][L] fp32, 16-byte aligned: prob[b][n][i][j] = softmax_j((ac + bd)[i][j] * d_head^-0.5) of session b,
 * head n -- the probabilities BEFORE the dropout on them, with the opt-in key_len mask applied (exact zeros at masked
 * columns, the diagonal kept).  The forward writes exactly these B n_head L L floats; the backward reads them instead of
 * recomputing the scores from q, k and k_r, and regenerates the dropout mask from (seed, ctr) as t4r_xlnet_attn_bwd does.
 * t4r_xlnet_layer_fwd / t4r_xlnet_layer_bwd do this inside a layer's workspace; these entries exist for callers that drive
 * the kernels one by one (and for the tests).
 */
#ifndef T4R_HIP_ATTN_H
#define T4R_HIP_ATTN_H

#ifdef __cplusplus
extern "C" {
#endif

/* t4r_xlnet_attn_block_fwd (t4r_hip.h: same arguments, same launch, the same bits in everything it writes) with `prob` after
 * `lse`.  prob null: nothing more is stored -- t4r_xlnet_attn_block_fwd itself. */
int t4r_xlnet_attn_block_fwd_prob(void* stream, const float* h, const float* planes, const float* o, const float* kr,
                                  long kr_bstride, const float* r_w_bias, const float* r_r_bias, const float* gamma,
                                  const float* beta, float* qkv, float* av, float* lse, float* prob, float* ao, float* mean,
                                  float* rstd, float* h1, int B, int L, int D, int n_head, float eps, float drop_p,
                                  unsigned long long seed, unsigned long long ctr_prob, unsigned long long ctr_out,
                                  const int* key_len);
/* t4r_xlnet_attn_bwd (t4r_hip.h) for L <= 32 and d_head 16 / 32, reading `prob` in place of `out`, `lse` and `key_len` (the
 * mask is in the probabilities).  Same outputs, same workspace (t4r_xlnet_attn_bwd_ws_floats), d_r_w_bias / d_r_r_bias
 * accumulated into; the results agree with t4r_xlnet_attn_bwd to fp32 rounding (the sums over sequence positions run over
 * fewer padded terms, in another order) and are the same bits from run to run.  Other shapes: an argument error. */
int t4r_xlnet_attn_bwd_prob(void* stream, const float* q, const float* k, const float* v, const float* k_r,
                            const float* r_w_bias, const float* r_r_bias, const float* prob, const float* dout, float* dq,
                            float* dk, float* dv, float* dk_r, float* d_r_w_bias, float* d_r_r_bias, float* workspace, int B,
                            int L, int n_head, int d_head, int kr_per_batch, float drop_p, unsigned long long seed,
                            unsigned long long ctr_hi);

#ifdef __cplusplus
}
#endif
#endif /* T4R_HIP_ATTN_H */
