// Every C++-linkage function of the library that crosses translation units, declared ONCE, and the small option structs of
// the internal entries.  (The extern "C" entries are declared by the public headers in include/: a translation unit that
// defines or calls one includes that header, so the compiler checks every definition and every call against it.)
#pragma once
#include "t4r_common.h"

struct GemmParams;   // gemm_kernel.h
struct GumbelCfg;    // gumbel_noise.h
struct ItkFilter;    // item_filter.h

// ------------------------------------------------------------------------------------------------ gemm_f32.hip
// Operand maxima of ONE launch (device words, one per workgroup of the kernel that produced the operand: a floats max |A|
// in na slots, max |B| in nb slots): a launch that would run in the three-plane bf16 form runs in the two-way fp16 form
// instead (gemm_kernel.h: PREC 4), positioned by them.
struct GemmAmax { const float* a; int na; const float* b; int nb; };
// Deterministic split-K (gemm_f32.hip): the sink is a value its OWNER holds, on the stack of one call, over `cap` floats of
// scratch; the launches that are handed it park partial tiles / register jobs, t4r_splitk_sink_flush adds them in ONE launch
struct SplitKJob { const float* part; float* out; int n4; int splits; long stride4; int accumulate; };
constexpr int kMaxSplitKJobs = 20;
struct SplitKJobs { SplitKJob j[kMaxSplitKJobs]; int n; int blk_end[kMaxSplitKJobs]; };
struct SplitKSink {
    float* ws; long cap, used = 0; SplitKJobs jobs; int bypassed = 0;   // bypassed: eligible launches that found no room (-> atomics)
    SplitKSink(float* ws_, long cap_floats) : ws(ws_), cap(ws_ ? cap_floats : 0) { jobs.n = 0; }
};
int t4r_splitk_sink_flush(SplitKSink& sink, hipStream_t st);
// what ONE launch may use beyond its operands: operand maxima; the sink of its split-K partial tiles (null: fp32 atomics)
struct GemmOpts { const GemmAmax* amax = nullptr; SplitKSink* sink = nullptr; };
// Where the second stage of a column reduction (t4r_reduce_partials_launch) goes: into `sink` (ACCUMULATED sums only); else
// onto `side`, after its first stage by events[used++] while events are left; else, as with a null ReduceCtx*, its own
// kernel on the caller's stream at once.  The XLNet layer backward holds one per call; every public entry passes null.
struct ReduceCtx { SplitKSink* sink = nullptr; hipStream_t side = nullptr; hipEvent_t* events = nullptr; int n_events = 0, used = 0; };
// the C++ entry of the composite (layer / head) launchers
int t4r_gemm_launch(hipStream_t stream, int transA, int transB, int M, int N, int K, float alpha,
                    const float* A, long lda, const float* B, long ldb, float* C, long ldc,
                    const float* bias, int epilogue, float* aux, long ldaux, int splitk,
                    int accumulate, int batch, long sA, long sB, long sC, const DropCfg* drop,
                    GemmOpts opt = GemmOpts());
int t4r_gemm_softmax_grad_launch(hipStream_t stream, int transA, int n_rows, int Vc, int V, int yoff, int N,
                                 float alpha, const float* logits, long ld_logits, const float* lse,
                                 const long* labels, const float* grad_out, float label_smoothing, const float* B,
                                 long ldb, float* C, long ldc, int splitk, int accumulate);
int t4r_gemm_fp32_nt_launch(hipStream_t stream, int M, int N, int K, float alpha, const float* A, long lda,
                            const float* B, long ldb, float* C, long ldc);
int t4r_gemm_topk_collect_launch(hipStream_t stream, int n_rows, int V, int D, float alpha, const float* X, long ldx,
                                 const float* W, long ldw, const float* thr, long thr_ld, int* count, float* cand_val,
                                 int* cand_idx, int cap, const GumbelCfg* noise);
int t4r_gemm_topk_collect_filtered_launch(hipStream_t stream, int n_rows, int V, int D, float alpha, const float* X, long ldx,
                                          const float* W, long ldw, const float* thr, long thr_ld, int* count, float* cand_val,
                                          int* cand_idx, int cap, const GumbelCfg* noise, const ItkFilter* filt);
bool t4r_splitk_sink_add_reduce(SplitKSink& sink, const float* part, int nblocks, int n, float* const* outs, const int* lens,
                                const int* accs, int n_seg);
int t4r_gemm_half_dispatch(const GemmParams& p, int batch, int ta, int tb, int bm, int bn, int prec, hipStream_t stream);   // gemm_half.hip
int t4r_tok_gemm_try(const GemmParams& p, int batch, int ta, int tb, hipStream_t stream);                                  // tok_gemm.hip

// ------------------------------------------------------------------------------------------------ elementwise.hip, head.hip
int t4r_reduce_partials_launch(hipStream_t st, const float* part, int nblocks, float* o0, int n0, int a0,
                               float* o1, int n1, int a1, float* o2, int n2, int a2, ReduceCtx* red);
// t4r_add_layernorm_bwd (include/t4r_hip.h) and the launcher under t4r_act_bwd_bias (mode 0 / 1) and t4r_colsum (mode 2, no
// pre / dpre), with the context of their second stage
int t4r_add_layernorm_bwd_impl(void* stream, const float* a, const float* b, const float* gamma, const float* mean,
                               const float* rstd, const float* dy, float* dx, float* dxa, float* dgamma, float* dbeta,
                               float* ws, int rows, int D, int accumulate_dx, float drop_p, unsigned long long seed,
                               unsigned long long ctr_hi, ReduceCtx* red);
int t4r_colred_launch(hipStream_t st, const float* dact, const float* pre, float* dpre, float* dbias, float* ws, long rows,
                      int N, long ld, int mode, DropCfg drop, ReduceCtx* red);
int t4r_mean_launch(hipStream_t stream, const float* x, int n, float* out);

// ------------------------------------------------------------------------------------------------ xlnet_fused.hip
// token blocks (of 16 rows) per workgroup tile of the token-tile kernels for T rows.  backward = true: the launch may run
// next to a resident collective -- the CU budget of t4r_xlnet_set_cu_budget applies (forward launches never do)
int t4r_xlnet_pick_r(long T, bool backward);
bool t4r_xlnet_body_fp16x2();      // the token-tile kernels on the two-way fp16 split (T4R_XLNET_FP16X2, default 1)?
int t4r_xlnet_ff_amax_count(long T);         // workgroups (= maxima slots written) of a feed-forward forward launch on T rows
int t4r_xlnet_ff_amax_count_bwd(long T);     // ... of a backward launch
long t4r_xlnet_ff_amax_slots(long T);        // upper bound of both
// What the layer asks of its feed-forward launches beyond the public entries (which pass FFOpts()):
//   amax0 / amax1  where the launch leaves its per-workgroup operand maxima, t4r_xlnet_ff_amax_slots(T) floats each: max |h1|,
//                  max |act| (forward) or max |d pre|, max |d ffout| (backward).  The two feed-forward weight-gradient
//                  launches then run in the two-way fp16 form (GemmAmax).  Null: not stored.
//   final_on / final_ctr  the launch also applies the model-level output dropout keyed by final_ctr (the last layer of a
//                  stack: one launch less per direction and no extra pass over [T, D])
//   red            (backward) where the second stages of the bias / LayerNorm-2 gradient sums go (ReduceCtx above)
struct FFOpts {
    float* amax0 = nullptr; float* amax1 = nullptr; int final_on = 0; unsigned long long final_ctr = 0; ReduceCtx* red = nullptr;
};
// t4r_xlnet_ff_fwd / _bwd (include/t4r_hip.h) and their row-mapped forms (include/t4r_hip_rows.h: rows != null) in one
int t4r_xlnet_ff_fwd_impl(void* stream, const float* h1, const float* planes, const float* b1, const float* b2,
                          const float* gamma, const float* beta, float* ffpre, float* ffact, float* ffout, float* mean,
                          float* rstd, float* hout, int T, int D, float eps, float drop_p, unsigned long long seed,
                          unsigned long long ctr_act, unsigned long long ctr_out, const int* rows, int n, const FFOpts& opt);
int t4r_xlnet_ff_bwd_impl(void* stream, const float* dy, const float* ffout, const float* h1, const float* mean,
                          const float* rstd, const float* gamma, const float* ffpre, const float* planes,
                          float* dh1, float* dffout, float* dpre, float* d_gamma, float* d_beta,
                          float* d_b2, float* d_b1, float* part, int T, int D, float drop_p,
                          unsigned long long seed, unsigned long long ctr_act, unsigned long long ctr_out,
                          const int* rows, int n, float* h1_rows, const FFOpts& opt);

// ------------------------------------------------------------------------------------------------ xlnet_fused_attn.hip
// t4r_xlnet_dh (include/t4r_hip.h) that masks its result with drop_in (the model-level input dropout of a first layer,
// T4R_LAYER_FUSE_INPUT; p = 0: off, the public entry)
// t4r_xlnet_ln1_bwd (include/t4r_hip.h) and t4r_xlnet_ln1_bwd_rows (include/t4r_hip_rows.h) with the context of their
// d gamma / d beta second stage
int t4r_xlnet_ln1_bwd_impl(void* stream, const float* dy, const float* ao, const float* h, const float* mean, const float* rstd,
                           const float* gamma, const float* planes, float* dh, float* dao, float* dav, float* d_gamma,
                           float* d_beta, float* part, long T, int D, float drop_p, unsigned long long seed,
                           unsigned long long ctr_hi, ReduceCtx* red);
int t4r_xlnet_ln1_bwd_rows_impl(void* stream, const float* dy, const float* ao, const float* h, const float* mean,
                                const float* rstd, const float* gamma, const float* planes, float* dh, float* dao, float* dav,
                                float* d_gamma, float* d_beta, float* part, long T, int D, float drop_p, unsigned long long seed,
                                unsigned long long ctr_hi, const int* rows, int n, ReduceCtx* red);
int t4r_xlnet_dh_impl(void* stream, const float* dqkv, const float* planes, float* dh, long T, int D, const DropCfg& drop_in);

// ------------------------------------------------------------------------------------------------ xlnet_attn_block.hip
// t4r_xlnet_attn_block_fwd (include/t4r_hip.h) plus
//   prob   null, or [B][n_head][L][L] fp32, 16-byte aligned: the attention probabilities before dropout (exact zeros at
//          masked columns) are stored there for the core's backward
//   in_on  the kernel applies the model-level input dropout keyed by in_ctr to h on load and leaves the dropped rows in hin
//          [T, D] (the first layer of a stack, T4R_LAYER_FUSE_INPUT)
int t4r_xlnet_attn_block_fwd_impl(void* stream, const float* h, const float* planes, const float* o, const float* kr,
                                  long kr_bstride, const float* r_w_bias, const float* r_r_bias, const float* gamma,
                                  const float* beta, float* qkv, float* av, float* lse, float* prob, float* ao, float* mean,
                                  float* rstd, float* h1, int B, int L, int D, int n_head, float eps, float drop_p,
                                  unsigned long long seed, unsigned long long ctr_prob, unsigned long long ctr_out,
                                  const int* key_len, int in_on, unsigned long long in_ctr, float* hin);

// ------------------------------------------------------------------------------------------------ xlnet_attn*.hip
// t4r_xlnet_attn_bwd (include/t4r_hip.h) plus prob: null, or the probabilities the one-kernel forward stored (the one-wave
// matrix-core kernel then reads them instead of recomputing the scores; lse is not read and may be null)
int t4r_xlnet_attn_bwd_impl(void* stream, const float* q, const float* k, const float* v, const float* k_r,
                            const float* r_w_bias, const float* r_r_bias, const float* out, const float* lse,
                            const float* prob, const float* dout, float* dq, float* dk, float* dv, float* dk_r,
                            float* d_r_w_bias, float* d_r_r_bias, float* workspace, int B, int L, int n_head, int d_head,
                            int kr_per_batch, float drop_p, unsigned long long seed, unsigned long long ctr_hi,
                            const int* key_len, ReduceCtx* red);
extern "C" int t4r_xlnet_attn_bwd_blocks(int B);      // xlnet_attn.hip; not part of the public ABI headers
// general kernels (xlnet_attn_long.hip): any L, d_head up to 256
int t4r_xlnet_attn_long_ok(int L, int d_head);
int t4r_xlnet_attn_long_fwd(hipStream_t st, const float* q, const float* k, const float* v, const float* kr, const float* rw,
                            const float* rr, float* out, float* lse, int B, int L, int n_head, int d_head, float scale,
                            long kr_bstride, DropCfg drop, const int* key_len);
int t4r_xlnet_attn_long_bwd(hipStream_t st, const float* q, const float* k, const float* v, const float* kr, const float* rw,
                            const float* rr, const float* out, const float* lse, const float* dout, float* dq, float* dk,
                            float* dv, float* part, float* delta, float* dkr, float* d_rw, float* d_rr, int B, int L, int n_head,
                            int d_head, float scale, long kr_bstride, DropCfg drop, const int* key_len, ReduceCtx* red);
// t4r_xlnet_attn_uni_bwd (include/t4r_hip_uni.h: the causal core, xlnet_attn_uni.hip) with the context of its second stage
int t4r_xlnet_attn_uni_bwd_impl(void* stream, const float* q, const float* k, const float* v, const float* k_r,
                                const float* r_w_bias, const float* r_r_bias, const float* out, const float* lse,
                                const float* dout, float* dq, float* dk, float* dv, float* dk_r, float* d_r_w_bias,
                                float* d_r_r_bias, float* workspace, int B, int L, int n_head, int d_head, int kr_per_batch,
                                float drop_p, unsigned long long seed, unsigned long long ctr_hi, const int* key_len,
                                ReduceCtx* red);
// MFMA kernels for L <= 32, d_head 16 / 32 (xlnet_attn_mfma.hip); T4R_ATTN_MFMA=0 keeps the VALU kernels
int t4r_xlnet_attn_mfma_ok(int L, int d_head);
int t4r_xlnet_attn_mfma_fwd(hipStream_t st, const float* q, const float* k, const float* v, const float* kr,
                            const float* rw, const float* rr, float* out, float* lse, int B, int L, int n_head,
                            int d_head, float scale, long kr_bstride, DropCfg drop, const int* key_len);
int t4r_xlnet_attn_mfma_bwd(hipStream_t st, const float* q, const float* k, const float* v, const float* kr,
                            const float* rw, const float* rr, const float* lse, const float* prob, const float* dout,
                            float* dq, float* dk, float* dv, float* part, float* dkr, float* d_rw, float* d_rr, int B,
                            int L, int n_head, int d_head, float scale, long kr_bstride, DropCfg drop, const int* key_len,
                            ReduceCtx* red);

// ------------------------------------------------------------------------------------------------ mha*.hip
// mha_mfma.hip: matrix-core kernels for d_head 32 / 64
bool t4r_mha_mfma_ok(int L, int d_head, long ld, long ld_out, long ld_d);
int t4r_mha_mfma_fwd(hipStream_t st, const float* q, const float* k, const float* v, long ld, float* out,
                     long ld_out, float* lse, int B, int L, int n_head, int d_head, float scale, int causal,
                     DropCfg drop, const int* key_len);
int t4r_mha_mfma_bwd(hipStream_t st, const float* q, const float* k, const float* v, long ld, const float* out,
                     const float* dout, long ld_out, const float* lse, float* dq, float* dk, float* dv, long ld_d,
                     int B, int L, int n_head, int d_head, float scale, int causal, DropCfg drop, const int* key_len);
// general kernels (xlnet_attn_long.hip): any L, d_head up to 256
int t4r_mha_long_ok(int L, int d_head);
int t4r_mha_long_fwd(hipStream_t st, const float* q, const float* k, const float* v, long ld, float* out, long ld_out, float* lse,
                     int B, int L, int n_head, int d_head, float scale, int causal, DropCfg drop, const int* key_len);
int t4r_mha_long_bwd(hipStream_t st, const float* q, const float* k, const float* v, long ld, const float* out, const float* dout,
                     long ld_out, const float* lse, float* dq, float* dk, float* dv, long ld_d, int B, int L, int n_head,
                     int d_head, float scale, int causal, DropCfg drop, const int* key_len);

#ifdef T4R_EXPERIMENTAL     /* tools/experimental: measured slower, compiled only into the A/B variant library */
// wgrad_stream.hip: the K-streaming weight-gradient kernel
void t4r_wgrad_stream_plan(int K, int* splits, int* kper);
bool t4r_wgrad_stream_ok(const GemmParams& p);
int t4r_wgrad_stream_launch(const GemmParams& p, int batch, int kper, float* part, hipStream_t st);
// wgrad_units.hip: read-once, cut-once 128 x 128 units in the two-way fp16 form (T4R_WGRAD_UNITS=1)
void t4r_wgrad_units_plan(int K, int* splits, int* kper);
bool t4r_wgrad_units_ok(const GemmParams& p);
int t4r_wgrad_units_launch(const GemmParams& p, int batch, int kper, float* part, hipStream_t st);
// the fp32-MFMA attention core with the permuted k-slots (phase 3 of the one-kernel backward as its own launch)
int t4r_xlnet_attn_core16_ok(int L, int D, int n_head);
int t4r_xlnet_attn_core16_bwd(hipStream_t st, const float* qkv, const float* kr, const float* rw, const float* rr,
                              const float* lse, const float* dout, float* dqkv, float* part, float* dkr, float* d_rw,
                              float* d_rr, int B, int L, int n_head, int d_head, float scale, long kr_bstride, DropCfg drop,
                              const int* key_len, ReduceCtx* red);
// the one-kernel backward of the attention half (xlnet_attn_block_bwd.inc)
extern "C" long t4r_xlnet_attn_block_bwd_part_floats(int B, int L, int D, int n_head);
int t4r_xlnet_attn_block_bwd_impl(void* stream, const float* dh1, const float* ao, const float* h, const float* mean,
                                  const float* rstd, const float* gamma, const float* planes, const float* wq,
                                  const float* wk, const float* wv, const float* qkv, const float* kr, long kr_bstride,
                                  const float* r_w_bias, const float* r_r_bias, const float* lse, float* dh, float* dao,
                                  float* dqkv, float* dkr, float* d_rw, float* d_rr, float* d_gamma, float* d_beta,
                                  float* part, int B, int L, int D, int n_head, float drop_p, unsigned long long seed,
                                  unsigned long long ctr_prob, unsigned long long ctr_out, const int* key_len, ReduceCtx* red);
#endif
