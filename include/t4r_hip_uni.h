/* t4r_hip_uni.h -- XLNet with attn_type = "uni": the causal relative-attention core and the layer around it.  An EXTENSION
 * header of libt4r_hip.so (transformers4rec_amd/_lib.py: EXTENSION_HEADERS): same library, same conventions as t4r_hip.h (device
 * pointers, float = fp32, long = int64, `stream` a hipStream_t, nothing synchronises, nothing is allocated or copied, argument
 * errors -- checked before any launch -- come back non-zero with t4r_last_error() for the message, no state kept between calls).
 *
 * What "uni" is (HF modeling_xlnet.py create_mask :895-925, relative_positional_encoding :940-976, rel_shift_bnij :81-93): key
 * j of query row i is masked when j > i, and the relative encoding keeps the positions L .. 0 -- the first L + 1 rows of the
 * "bi" encoding.  A live pair (j <= i) meets row m = j - i + L, in [1, L], of the SAME [2 L, D] array k_r that the bi entries
 * take.  So every entry here has the arguments, buffers and workspaces of its bi namesake in t4r_hip.h, and differs in the dead
 * set alone: key j of row i is dead when j > i, or when key_len != NULL && j >= key_len[b] && j != i (the opt-in padding rule,
 * unclamped).  A dead key has probability exactly 0 in the forward and in every gradient.  Rows 0 and L + 1 .. 2 L - 1 of k_r
 * are never read, and the same rows of dk_r are written as exact zeros.  Dropout: the bi kernels' key and element index
 * ((b n_head + h) L + i) L + j, so the masks are those of the bi entries.
 */
#ifndef T4R_HIP_UNI_H
#define T4R_HIP_UNI_H

#ifdef __cplusplus
extern "C" {
#endif

/* t4r_xlnet_attn_fwd / t4r_xlnet_attn_bwd (t4r_hip.h) with the causal dead set.  Any L >= 1, any d_head in [1, 256] (16-byte
 * requests when d_head % 4 == 0, element by element otherwise).  backward: d_r_w_bias / d_r_r_bias ACCUMULATED, the rest
 * overwritten; workspace: t4r_xlnet_attn_bwd_ws_floats(B, L, n_head d_head, n_head) floats; the batch-reduced gradients go
 * through per-workgroup partial sums added in a fixed order (the same bits from run to run). */
int t4r_xlnet_attn_uni_fwd(void* stream, const float* q, const float* k, const float* v, const float* k_r,
                           const float* r_w_bias, const float* r_r_bias, float* out, float* lse, int B,
                           int L, int n_head, int d_head, int kr_per_batch, float drop_p,
                           unsigned long long seed, unsigned long long ctr_hi, const int* key_len);
int t4r_xlnet_attn_uni_bwd(void* stream, const float* q, const float* k, const float* v, const float* k_r,
                           const float* r_w_bias, const float* r_r_bias, const float* out,
                           const float* lse, const float* dout, float* dq, float* dk, float* dv,
                           float* dk_r, float* d_r_w_bias, float* d_r_r_bias, float* workspace, int B,
                           int L, int n_head, int d_head, int kr_per_batch, float drop_p,
                           unsigned long long seed, unsigned long long ctr_hi, const int* key_len);

/* t4r_xlnet_layer_fwd / t4r_xlnet_layer_bwd (t4r_hip.h) with the causal core: same parameters, `ws` of
 * t4r_xlnet_layer_ws_floats and `bws` of t4r_xlnet_layer_bwd_ws_floats floats, same dropout keys at every site, pos_emb still
 * the [2 L, D] encoding (all 2 L rows are projected; the core reads rows 1 .. L).  The q | k | v projection, the o-projection +
 * LayerNorm, the feed-forward block, the weight gradients, the deferred join and a prepared stack (T4R_LAYER_STACK_PREPARED)
 * are those of the bi layer.  The attention half always runs as projection -> core -> o-projection (never the one-kernel
 * attention block, never the stored probabilities); T4R_LAYER_FUSE_INPUT in layer_idx is an argument error. */
int t4r_xlnet_layer_uni_fwd(void* stream, const float* h, const float* pos_emb, const float* const* params, float* ws,
                            float* h_out, int B, int L, int D, int n_head, float ln_eps, float drop_p,
                            unsigned long long seed, unsigned long long offset, int layer_idx, const int* key_len,
                            const float* pos_emb_b);
int t4r_xlnet_layer_uni_bwd(void* stream, const float* h, const float* pos_emb, const float* const* params,
                            float* const* grads, const float* ws, float* bws, const float* dh_out, float* dh_in, int B, int L,
                            int D, int n_head, float ln_eps, float drop_p, unsigned long long seed,
                            unsigned long long offset, int layer_idx, const int* key_len, const float* pos_emb_b);

#ifdef __cplusplus
}
#endif
#endif /* T4R_HIP_UNI_H */
