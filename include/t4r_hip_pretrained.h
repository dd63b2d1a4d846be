/* t4r_hip_pretrained.h -- the pretrained-embedding entries of libt4r_hip.so: a frozen table of item vectors kept on the device
 * as an fp16 image (t4r_item_table_pack_h16 of t4r_hip.h: rows 16-byte aligned, pad columns zero) is gathered by id INSIDE the
 * kernel that projects it, forward and backward; the gathered [T, E] rows never visit HBM.  The conventions are t4r_hip.h's
 * (device pointers unless marked "host", float = fp32, long = int64, `stream` a hipStream_t, nothing synchronises, nothing is
 * allocated or copied, argument errors -- checked before any launch -- come back negative with t4r_last_error() for the message,
 * no state kept between calls).
 * Reference paths are relative to the reference repository root (NVIDIA-Merlin/Transformers4Rec).
 *
 * replaces: PretrainedEmbeddingFeatures.forward (transformers4rec/torch/features/embedding.py:599-740) for one feature -- the
 * torch.nn.Linear of `projection` and the torch.nn.LayerNorm of `post.feature_layer_norm` on rows the data loader looked up.
 *
 * Arithmetic contract of the forward.  The gathered operand is exactly an fp16 value, so only W is cut:
 *     m = max |W|,  c = 2^k with m * c in [2^14, 2^15)  (k clamped to <= 126; c = 1 for m = 0)
 *     hi = fp16(W * c),  lo = fp16(W * c - hi)          (both roundings to nearest even; W * c and the difference are exact)
 *     z[t, p] = (sum over k-steps of 16 columns, ascending: hi . x, then lo . x, each one v_mfma_f32_32x32x16_f16 into the same
 *               fp32 accumulator) / c + b[p]
 * and, with gamma / beta given, xhat = (z - mean) * rstd with mean, var over the P outputs in fp32 (two passes), rstd =
 * 1 / sqrt(var + eps), out = xhat * gamma + beta.  A row's bits depend on its id and the parameters only: not on its position,
 * on T or on the launch shape.
 */
#ifndef T4R_HIP_PRETRAINED_H
#define T4R_HIP_PRETRAINED_H

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the forward's workspace: 256 + ceil(P / 32) * ceil(E / 16) * 2048 (a header with the scale, then the hi | lo planes
 * of W in matrix-operand order).  A pure function, non-decreasing in E and in P; 0 outside 1 <= E <= 1024, 1 <= P <= 256. */
long t4r_pretrained_proj_ws_bytes(int E, int P);
/* For token t < T, id = ids[t / ids_div]:   out[t, col : col + P] = LN?( float(image[id, :E]) . W^T + b ).
 *   dtype    3 (fp16, the code of T4R_GEMM_PREC); a bf16 image (2) is refused
 *   image    [rows, ldp] fp16, 16-byte aligned, ldp % 8 == 0, ldp >= t4r_item_table_image_ld(E), pad columns zero; read only.
 *            Row 0 is read like any other row.
 *   ids      int64 [T / ids_div]; ids_div >= 1 divides T (ids_div = L: a per-session [B] id broadcast over the sequence).  An id
 *            outside [0, rows) sets *err_flag = 1 (err_flag may be null) and reads row 0 instead.
 *   W [P, E], b [P] fp32 (b may be null: no bias).  gamma, beta [P]: both null (no LayerNorm) or both given.
 *   out      [T, ld_out] fp32, ld_out >= col + P; only columns [col, col + P) are written.
 *   xhat     null, or [T, P] fp32: with LayerNorm the NORMALISED row (before gamma / beta), what t4r_pretrained_proj_bwd reads.
 *   rstd     null, or [T] fp32: with LayerNorm 1 / sqrt(var + eps).  Neither is touched without LayerNorm.
 *   ws       t4r_pretrained_proj_ws_bytes(E, P) bytes, 16-byte aligned; filled by a prologue launch of this call, all of it the
 *            kernel's, nothing in it is read from an earlier call.
 * 1 <= E <= 1024, 1 <= P <= 256, 1 <= rows < 2^31, 0 <= T < 2^31 (T = 0: nothing launches).  0 on success. */
int t4r_pretrained_proj_fwd(void* stream, int dtype, const void* image, long ldp, long rows, const long* ids, long T, int ids_div,
                            const float* W, const float* b, const float* gamma, const float* beta, float eps, int E, int P,
                            float* out, long ld_out, int col, float* xhat, float* rstd, void* ws, int* err_flag);
/* Floats of the backward's workspace: S * roundup(P, 32) * roundup(E, 128) + roundup(T * P, 4) + S * 6 * P with
 * S = min(max(ceil(T / 64), 1), 128) token chunks.  A pure function, non-decreasing in each argument; 0 outside the limits. */
long t4r_pretrained_proj_bwd_ws_floats(long T, int E, int P);
/* The gradients of t4r_pretrained_proj_fwd's parameters from dY = columns [col, col + P) of the aggregate's gradient [T, ld];
 * there is no gradient for the table.  With gamma (then xhat and rstd of the forward are required):
 *     g = dY * gamma,  dZ = rstd * (g - mean(g) - xhat * mean(g * xhat)),  dgamma += sum_t dY * xhat,  dbeta += sum_t dY
 * without: dZ = dY.  Then db += sum_t dZ and dW[P, E] += dZ^T . X with X gathered again from the image (ids as in the forward; an
 * id out of range reads row 0) and multiplied exactly: v_mfma_f32_32x32x2_f32 on fp32 dZ and the fp16 values widened to fp32.
 * Every output is ACCUMULATED; dW, db, dgamma, dbeta may each be null.  The sums over tokens are taken in S chunks of
 * ceil(T / S) consecutive tokens, inside a chunk in a fixed order, and the S partials are added in chunk order: no float
 * atomics, the same bits from run to run.  The three column sums (db, dgamma, dbeta) are accumulated in double and rounded to
 * fp32 once, at the end; d W accumulates in the fp32 accumulators of the matrix instruction.
 *   ws   t4r_pretrained_proj_bwd_ws_floats(T, E, P) floats, 16-byte aligned.
 * Limits as the forward.  0 on success. */
int t4r_pretrained_proj_bwd(void* stream, int dtype, const void* image, long ldp, long rows, const long* ids, long T, int ids_div,
                            const float* dY, long ld, int col, const float* gamma, const float* xhat, const float* rstd,
                            int E, int P, float* dW, float* db, float* dgamma, float* dbeta, float* ws);

#ifdef __cplusplus
}
#endif
#endif /* T4R_HIP_PRETRAINED_H */
