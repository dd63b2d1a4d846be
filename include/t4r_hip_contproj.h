/* t4r_hip_contproj.h -- the continuous-feature projection of libt4r_hip.so: the first layer of the MLP that
 * `continuous_projection` puts over the concatenated continuous columns, computed from the separate column tensors.  The
 * conventions are t4r_hip.h's (device pointers unless marked "host", float = fp32, long = int64, `stream` a hipStream_t, nothing
 * synchronises, nothing is allocated or copied, argument errors -- checked before any launch -- come back negative with
 * t4r_last_error() for the message, no state kept between calls).
 * Reference paths are relative to the reference repository root (NVIDIA-Merlin/Transformers4Rec).
 *
 * The reference builds SequentialBlock(ContinuousFeatures(aggregation="concat"), MLPBlock(dims), AsTabular(...))
 * (transformers4rec/torch/features/tabular.py:90-117, features/sequence.py:271-284): every column is unsqueezed to [B, L, 1]
 * (features/continuous.py:60-63), the C columns are concatenated in sorted-name order into [B, L, C]
 * (tabular/aggregation.py:35-47), and each MLP layer is ReLU(Linear(in, out)) (block/mlp.py:68-143).  Here the [T, C] operand
 * (T = B * L tokens) is never written: column c is read from its own tensor, [B, L] or -- a per-session feature, broadcast over
 * the sequence -- [B].  Layers after the first are ordinary GEMMs (t4r_gemm_f32 with the bias + ReLU epilogue).
 *
 * Limits: 1 <= C <= 64 columns, 1 <= P <= 1024 outputs, any ntok >= 0 below 2^31.
 */
#ifndef T4R_HIP_CONTPROJ_H
#define T4R_HIP_CONTPROJ_H

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when (C, P) is within the limits above, else 0.  No launch. */
int t4r_cont_proj_supported(int C, int P);
/* Floats of workspace t4r_cont_proj_bwd needs for ntok tokens: one [P, C + 1] partial per token chunk.  A pure function of its
 * arguments, non-decreasing in ntok and P; 0 for ntok <= 0 or (C, P) outside the limits.  No launch. */
long t4r_cont_proj_bwd_ws_floats(long ntok, int C, int P);
/* replaces: ConcatFeatures over the continuous columns + the first DenseBlock of MLPBlock(dims)
 * (transformers4rec/torch/tabular/aggregation.py:35-47, block/mlp.py:68-143: torch.nn.Linear + torch.nn.ReLU).
 * xs: host array of C device pointers, column c [ntok] fp32 or, where per_session[c] != 0 (host array of C ints), [ntok / L]
 * fp32 with value t / L serving token t.  W [P, C], b [P] fp32 (torch.nn.Linear's layout).  out [ntok, P] fp32, dense:
 *     out[t][p] = max(0, b[p] + sum_c W[p][c] * x_c[t]),
 * one chain of fp32 fused multiply-adds starting from b[p], c ascending: the same bits wherever the token sits in the launch.
 * A padded position (every x_c = 0) therefore comes out as max(0, b[p]), as in the reference.  16-byte stores when P % 4 == 0
 * and out is 16-byte aligned, scalar ones otherwise (4-byte alignment is required).  One launch.
 * ntok = 0: nothing launches, returns 0.  L >= 1 divides ntok.  0 on success. */
int t4r_cont_proj_fwd(void* stream, const float* const* xs, const int* per_session, long ntok, int L, int C, int P, const float* W,
                      const float* b, float* out);
/* replaces: the autograd backward of the same torch.nn.Linear + torch.nn.ReLU (block/mlp.py:68-143) for its parameters; the
 * inputs are data and get no gradient.
 * dout: the gradient of out as columns [col, col + P) of rows of pitch ld floats (ld >= col + P; neither need be a multiple
 * of 4), read only.  xs, per_session, W, b as in the forward: the pre-activation is recomputed with the forward's arithmetic
 * and nothing has to be saved.  With g[t][p] = dout[t][col + p] where out[t][p] > 0 and 0 elsewhere (torch's ReLU gradient:
 * zero at exactly 0):
 *     d_w[p][c] += sum_t g[t][p] * x_c[t]        d_w [P, C], may be NULL
 *     d_b[p]    += sum_t g[t][p]                 d_b [P], may be NULL
 *     dpre[t][p] = g[t][p]                       dpre [ntok, P] dense, may be NULL
 * The sums are ACCUMULATED into d_w and d_b.  Token chunks are summed by one workgroup each in token order, their partials
 * -- in ws -- in chunk order: no float atomics, the same bits from run to run.
 * ws: at least t4r_cont_proj_bwd_ws_floats(ntok, C, P) floats, contents undefined before and after.  Two launches.
 * ntok = 0: nothing launches, returns 0.  0 on success. */
int t4r_cont_proj_bwd(void* stream, const float* dout, long ld, int col, const float* const* xs, const int* per_session, long ntok,
                      int L, int C, int P, const float* W, const float* b, float* d_w, float* d_b, float* dpre, float* ws);

#ifdef __cplusplus
}
#endif
#endif /* T4R_HIP_CONTPROJ_H */
