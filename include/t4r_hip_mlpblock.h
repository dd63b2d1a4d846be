/* t4r_hip_mlpblock.h -- the MLP block of libt4r_hip.so: a stack of 1 .. 4 dense layers (Linear, optional ReLU, optional dropout)
 * between the input features and the transformer, forward in ONE launch with the layer-to-layer hand-over on chip.  The
 * conventions are t4r_hip.h's (device pointers, float = fp32, long = int64, `stream` a hipStream_t, nothing synchronises, nothing
 * is allocated or copied, argument errors -- checked before any launch -- come back negative with t4r_last_error() for the
 * message, no state kept between calls).  A feature header: bound through _lib.FEATURE_HEADERS.
 * Reference paths are relative to the reference repository root (NVIDIA-Merlin/Transformers4Rec).
 *
 * The reference's MLPBlock (transformers4rec/torch/block/mlp.py) builds, per entry of `dimensions`, a DenseBlock =
 * torch.nn.Sequential(torch.nn.Linear(in, out, bias=use_bias), activation(), [normalization], [torch.nn.Dropout(dropout)]).
 *
 * Symbols: T = ntok token rows, n layers (1 <= n <= 4), layer i has W_i [N_i, K_i] and b_i [N_i] in torch.nn.Linear's layout,
 * K_0 the input width, K_i = N_{i-1}; x = a_{-1} [T, K_0] dense.  Per token row t:
 *     z_i[t][d] = b_i[d] + sum_k W_i[d][k] * a_{i-1}[t][k]     one chain of fp32 fused multiply-adds seeded with b_i[d] (0 without
 *                                                              a bias), k ASCENDING (k = 0, 1, 2, ...; where K_i is odd one more
 *                                                              fma(0, 0, z) closes the chain: it changes nothing but an exact -0,
 *                                                              which becomes +0)
 *     r_i       = relu ? max(z_i, 0) : z_i
 *     a_i[t][d] = drop_p > 0 ? r_i * m : r_i,   m = keep(seed, ctr_hi_i, t * N_i + d) ? fl(1 / (1 - drop_p)) : 0
 * keep is t4r_hip.h's dropout rule (the comment above t4r_dropout): Philox4x32-10, key = seed, counter = (index >> 2, ctr_hi),
 * component index & 3; ctr_hi_i = t4r_dropout_ctr_hi(offset, layer = i, site = 8 (T4R_SITE_MLP_BLOCK)).
 * The bits of a row of every a_i do not depend on ntok nor on where the row sits in the launch.
 *
 * Host arrays: N (n ints), W, b, acts, d_W, d_b (n device pointers each) are read on the host during the call and not kept.
 *
 * Limits: 1 <= n <= 4, 1 <= K_0 <= 1024, 1 <= N_i <= 512, any ntok >= 0 below 2^31, 0 <= drop_p < 1.  Every pointer is 4-byte
 * aligned; 16-byte requests are used for a row-major operand whose width is a multiple of 4 and whose base is 16-byte aligned,
 * single elements otherwise (the same bits either way).
 */
#ifndef T4R_HIP_MLPBLOCK_H
#define T4R_HIP_MLPBLOCK_H

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when (n, K0, N[0 .. n-1]) is within the limits above, else 0.  No launch. */
int t4r_mlp_stack_supported(int n, int K0, const int* N);
/* Floats of workspace t4r_mlp_stack_bwd needs: the rows dz_i [ntok, N_i] of every layer and the per-split partials of
 * [d W_i | d b_i].  A pure function of its arguments, non-decreasing in ntok; 0 for ntok <= 0 and for anything outside the
 * limits.  No launch.  (The forward needs no workspace.) */
long t4r_mlp_stack_bwd_ws_floats(long ntok, int n, int K0, const int* N);
/* replaces: MLPBlock.forward (transformers4rec/torch/block/mlp.py: per layer torch.nn.Linear, the activation, torch.nn.Dropout).
 * x [ntok, K0] dense.  b: NULL, or n pointers of which any may be NULL (no bias in that layer).
 * acts: NULL (inference: only out [ntok, N_{n-1}] = a_{n-1} is written, the intermediate activations stay on chip), or n
 * pointers [ntok, N_i] dense (training: every a_i is stored there for the backward; out must then be NULL or acts[n-1]).
 * relu: 0 or 1, for every layer.  drop_p > 0 applies dropout after every layer.
 * ONE launch for the whole stack.  ntok = 0: nothing launches, returns 0.  0 on success. */
int t4r_mlp_stack_fwd(void* stream, const float* x, const float* const* W, const float* const* b, float* const* acts, float* out,
                      long ntok, int n, int K0, const int* N, int relu, float drop_p, unsigned long long seed,
                      unsigned long long offset);
/* replaces: the autograd backward of the same chain (transformers4rec/torch/block/mlp.py: torch.nn.Dropout, the activation,
 * torch.nn.Linear, per layer in reverse).  dout [ntok, N_{n-1}] dense, read only.
 *     dz_i = da_i * gate_i,   da_{n-1} = dout,   da_{i-1}[t][k] = sum_d dz_i[t][d] * W_i[d][k]   (one fma chain from 0, d ascending)
 *     gate_i = relu ? (a_i > 0 ? s : 0) : (drop_p > 0 ? keep ? s : 0 : 1),  s = fl(1 / (1 - drop_p)): with ReLU the stored a_i
 *     says "positive and kept" and no mask is recomputed; without it the keep mask is.
 *     d_W[i][d][k] += sum_t dz_i[t][d] * a_{i-1}[t][k]      d_b[i][d] += sum_t dz_i[t][d]      tokens ascending within a split
 * acts: the n pointers the forward filled; acts[i] is read where relu != 0 and, for i < n - 1, where d_W[i + 1] is asked for
 * (other entries may be NULL).  x is read for d_W[0] only (else it may be NULL).
 * dx [ntok, K0] is overwritten; d_W[i] [N_i, K_i] and d_b[i] [N_i] are ACCUMULATED.  dx, the arrays d_W and d_b and each of
 * their entries may be NULL.  The batch sums go through per-split partials in ws, added in split order: no float atomics, the
 * same bits from run to run.
 * ws: at least t4r_mlp_stack_bwd_ws_floats(...) floats, contents undefined before and after.
 * At most three launches: the d-input chain of the whole stack (one), the partial products of every layer's [d W | d b] (one),
 * their sums (one).  ntok = 0: nothing launches, returns 0.  0 on success. */
int t4r_mlp_stack_bwd(void* stream, const float* dout, const float* x, const float* const* W, const float* const* acts, float* dx,
                      float* const* d_W, float* const* d_b, float* ws, long ntok, int n, int K0, const int* N, int relu,
                      float drop_p, unsigned long long seed, unsigned long long offset);

#ifdef __cplusplus
}
#endif
#endif /* T4R_HIP_MLPBLOCK_H */
