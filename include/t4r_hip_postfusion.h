/* t4r_hip_postfusion.h -- the post-context fusion (Latent Cross) of libt4r_hip.so: context that does not go through the sequence
 * model is projected to the model width and merged with the body's output right before the prediction task.  The conventions
 * are t4r_hip.h's (device pointers, float = fp32, long = int64, `stream` a hipStream_t, nothing synchronises, nothing is
 * allocated or copied, argument errors -- checked before any launch -- come back negative with t4r_last_error() for the
 * message, no state kept between calls).  A feature header: bound through _lib.FEATURE_HEADERS after the main and the
 * extension headers.
 * Reference paths are relative to the reference repository root (NVIDIA-Merlin/Transformers4Rec).
 *
 * The reference's PostContextFusion.forward (transformers4rec/torch/experimental.py:81-104) runs the sequential module, the
 * context module, and then either torch.cat([seq, ctx], axis=-1) (:92-93) or context_projection = torch.nn.Linear(C, D) (:77,
 * :89-90) followed by torch.multiply(seq, 1.0 + ctx) (:94-95) or seq + ctx (:96-97).  A 2-D context is meant to be repeated
 * over the sequence (:85-87; the reference reads an attribute it never sets there and raises): here the kernels read row t / L.
 *
 * Symbols: T = ntok tokens (B sessions of L positions), seq [T, D] fp32 dense, ctx fp32 dense, [T, C] or -- per_session != 0 --
 * [T / L, C] with row t / L serving token t (t' below), W [D, C] and b [D] in torch.nn.Linear's layout,
 *     p[t][d] = b[d] + sum_c W[d][c] * ctx[t'][c]      one chain of fp32 fused multiply-adds seeded with b[d], c ascending.
 * Modes: 0 MUL  out[t][d] = seq[t][d] * (1 + p[t][d])   (1 + p and the product are one fp32 rounding each)
 *        1 SUM  out[t][d] = seq[t][d] + p[t][d]
 *        2 CONCAT  out[t] = seq[t] | ctx[t'], width D + C; no parameters: W and b must be NULL.
 * The bits of an output row do not depend on ntok nor on where the row sits in the launch.
 *
 * Limits: 1 <= D <= 1024, 1 <= C <= 256, any ntok >= 0 below 2^31, L >= 1 divides ntok.  Every pointer is 4-byte aligned;
 * 16-byte requests are used when D % 4 == 0, C % 4 == 0 and every pointer is 16-byte aligned, single elements otherwise (the
 * same bits either way).
 */
#ifndef T4R_HIP_POSTFUSION_H
#define T4R_HIP_POSTFUSION_H

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when (D, C) is within the limits above, else 0.  No launch. */
int t4r_post_fusion_supported(int D, int C);
/* Floats of workspace t4r_post_fusion_bwd needs: the per-split partials of [d_w | d_b] and, for a session-level context of the
 * two projected modes, the per-token d ctx rows.  A pure function of its arguments, non-decreasing in ntok; 0 for ntok <= 0,
 * for CONCAT (no workspace) and for anything outside the limits (D, C, mode, L not dividing ntok).  No launch. */
long t4r_post_fusion_bwd_ws_floats(long ntok, int L, int D, int C, int mode, int per_session);
/* replaces: torch.cat (transformers4rec/torch/experimental.py:92-93), or context_projection + torch.multiply(seq, 1.0 + ctx) /
 * seq + ctx (experimental.py:89-97: torch.nn.Linear, add, multiply), and the repeat of a 2-D context (:85-87).
 * out [ntok, D] (MUL, SUM) or [ntok, D + C] (CONCAT), dense.  One launch.
 * ntok = 0: nothing launches, returns 0.  0 on success. */
int t4r_post_fusion_fwd(void* stream, const float* seq, const float* ctx, const float* W, const float* b, float* out, long ntok,
                        int L, int D, int C, int mode, int per_session);
/* replaces: the autograd backward of the same chain (transformers4rec/torch/experimental.py:85-97: repeat, torch.nn.Linear,
 * add, multiply / add / cat).  dout [ntok, Dout] dense (Dout = D, or D + C for CONCAT), read only.  p is
 * recomputed with the forward's arithmetic; nothing has to be saved.
 *     MUL: dseq = dout * (1 + p), g = dout * seq.        SUM: dseq = dout, g = dout.
 *     d_w[d][c] += sum_t g[t][d] * ctx[t'][c]             d_w [D, C], tokens ascending
 *     d_b[d]    += sum_t g[t][d]                          d_b [D]
 *     dctx[t'][c] = sum_d g[t][d] * W[d][c]               and, for a session-level context, summed over the L tokens of the
 *                                                         session in token order
 *     CONCAT: dseq = dout[:, :D], dctx = dout[:, D:] (a session-level context: summed over L in token order); d_w and d_b
 *     must be NULL.
 * d_w and d_b are ACCUMULATED; dseq [ntok, D] and dctx (ctx's shape) are overwritten.  Each of d_w, d_b, dseq, dctx may be
 * NULL (seq may be NULL where it is not read: SUM and CONCAT).  The batch sums go through per-split partials in ws, added in
 * split order: no float atomics, the same bits from run to run.
 * ws: at least t4r_post_fusion_bwd_ws_floats(...) floats, contents undefined before and after; may be NULL where that is 0.
 * At most three launches.  ntok = 0: nothing launches, returns 0.  0 on success. */
int t4r_post_fusion_bwd(void* stream, const float* dout, const float* seq, const float* ctx, const float* W, const float* b,
                        float* dseq, float* dctx, float* d_w, float* d_b, float* ws, long ntok, int L, int D, int C, int mode,
                        int per_session);

#ifdef __cplusplus
}
#endif
#endif /* T4R_HIP_POSTFUSION_H */
