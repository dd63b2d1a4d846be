/* t4r_hip_rtd.h -- the replaced-token-detection (RTD, ELECTRA) discriminator head of libt4r_hip.so: one logit per token and
 * the binary cross entropy over the attended tokens.  The conventions are t4r_hip.h's (device pointers, float = fp32,
 * long = int64, `stream` a hipStream_t, nothing synchronises, nothing is allocated or copied, argument errors -- checked
 * before any launch -- come back negative with t4r_last_error() for the message, no state kept between calls).
 *
 * The reference library (NVIDIA-Merlin/Transformers4Rec) stops at the replacement draw (torch/masking.py:
 * ReplacementLanguageModeling.get_fake_tokens); its paper configs name the discriminator's loss weight.  The arithmetic
 * here is HuggingFace transformers' ElectraForPreTraining (models/electra/modeling_electra.py): the op chain
 *     ElectraDiscriminatorPredictions: dense = torch.nn.Linear(D, D) -> ACT2FN[hidden_act] -> dense_prediction =
 *     torch.nn.Linear(D, 1) -> squeeze(-1);   loss: torch.nn.BCEWithLogitsLoss over logits[attention_mask == 1]
 * is about seven launches forward (two GEMMs, the activation, a boolean gather of logits and of labels, the loss, its
 * mean) and twice that backward, with three [T, D] round trips each way.  Here the forward is two launches and the
 * backward three, and no [T, D] tensor is kept from the forward for the backward.
 *
 * T tokens (B * L), torch.nn.Linear layouts: W1 [D, D] (row p = output feature), b1 [D], w2 [D], b2 [1].
 *     a_t[p] = b1[p] + sum_d W1[p][d] x_t[d]          an fp32 fma chain per (t, p) on the fp32 matrix cores, seeded with b1[p]
 *     h_t    = act(a_t)                               act 0: erf-GELU (HF "gelu"), act 1: ReLU
 *     z_t    = b2 + sum_p w2[p] h_t[p]
 *     row_t  = max(z_t, 0) - z_t y_t + log1p(exp(-|z_t|))            torch's stable binary_cross_entropy_with_logits
 *     n      = sum_t active_t                         (active NULL: n = T)
 *     loss   = (1 / n) sum_{active} row_t
 * DIFFERENCE from HF: n = 0 (no active token) gives loss = 0 and all-zero gradients; HF's mean over an empty selection is NaN.
 * Determinism: no float atomics, every sum in one fixed order, the same bits from run to run; z_t and dx_t are the same bits
 * wherever token t sits in the launch, whatever T is (dx through the one factor g / n), and whichever of the 16-byte and
 * 4-byte access paths runs.
 *
 * Limits: D a multiple of 16, 16 <= D <= 512; 0 <= T < 2^31.
 */
#ifndef T4R_HIP_RTD_H
#define T4R_HIP_RTD_H

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when D is within the limits above, else 0.  No launch. */
int t4r_rtd_head_supported(int D);
/* Floats of workspace t4r_rtd_head_fwd and t4r_rtd_head_bwd need for ntok tokens: the backward's d a [ntok, D], one
 * [2 D + 4] partial per chunk of 128 tokens, and the d W1 partial tiles (at most max(D^2, 4 Mi) floats); the forward uses the
 * first ntok floats.  A pure function of its arguments, non-decreasing in ntok and D; 0 for ntok <= 0 or an unsupported D.
 * No launch. */
long t4r_rtd_head_ws_floats(long ntok, int D);
/* replaces: ElectraDiscriminatorPredictions.forward + BCEWithLogitsLoss over the active positions
 * (transformers/models/electra/modeling_electra.py: ElectraDiscriminatorPredictions, ElectraForPreTraining.forward).
 * x [T, D] fp32 dense, the discriminator body's output.  active: uint8 [T] (non-zero = attended) or NULL (every token).
 * label: uint8 [T] (non-zero = replaced) or NULL.  z [T] is written for EVERY token, inactive ones included.  With labels,
 * n_active[0] (int32) and loss[0] are written on the device and ws[0 .. T) holds the row losses (0 at inactive tokens)
 * afterwards; with label NULL (inference) only z is written and n_active, loss and ws may be NULL.
 * 16-byte accesses when x and W1 are 16-byte aligned, 4-byte ones otherwise (4-byte alignment is required); the same bits.
 * ws: at least t4r_rtd_head_ws_floats(T, D) floats.  Two launches (one for inference).
 * T = 0: nothing launches, returns 0.  0 on success. */
int t4r_rtd_head_fwd(void* stream, const float* x, const unsigned char* active, const unsigned char* label, long T, int D,
                     const float* W1, const float* b1, const float* w2, const float* b2, int act, float* z, int* n_active,
                     float* loss, float* ws);
/* replaces: the autograd backward of the same chain.  g: device [1], the upstream gradient of loss.  z, n_active: what the
 * forward wrote; x, active, label, W1, b1, w2, act as in the forward.
 *     dz_t = active_t (g / n) (sigmoid(z_t) - y_t)            n = 0: dz = 0
 *     da_t = (dz_t w2) * act'(a_t)                            a_t recomputed with the forward's instructions: the same bits
 *     dx_t = W1^T da_t                                        dx [T, D]: EVERY element is written; inactive rows are 0
 *     d_W1[p][d] += sum_t da_t[p] x_t[d]     d_b1 += sum_t da_t     d_w2[p] += sum_t dz_t h_t[p]     d_b2 += sum_t dz_t
 * The parameter sums are ACCUMULATED, and each of d_W1 [D, D], d_b1 [D], d_w2 [D], d_b2 [1] may be NULL.  d_W1: splits of
 * the token range are summed in token order by one wave per 64 x 64 tile, the partial tiles -- in ws -- in split order;
 * the others: the 128 tokens of a chunk by one workgroup (a fixed butterfly over each wave's 32 tokens, the four waves in
 * token order), the chunk partials in chunk order.
 * ws: at least t4r_rtd_head_ws_floats(T, D) floats; 16-byte accesses to it need it 16-byte aligned (as x and W1).  Its
 * content afterwards is undefined.  Three launches (two without d_W1, one without any parameter gradient).
 * T = 0: nothing launches, returns 0.  0 on success. */
int t4r_rtd_head_bwd(void* stream, const float* g, const float* x, const unsigned char* active, const unsigned char* label,
                     const float* z, const int* n_active, long T, int D, const float* W1, const float* b1, const float* w2,
                     int act, float* dx, float* d_W1, float* d_b1, float* d_w2, float* d_b2, float* ws);

#ifdef __cplusplus
}
#endif
#endif /* T4R_HIP_RTD_H */
