// Host side of the GEMM: tile / split-K / precision selection and the C ABI entry points.
// The kernel template lives in gemm_kernel.h (shared with gemm_half.hip, which instantiates the
// bf16 / fp16 matrix-core variants in its own translation unit).
#include "gemm_kernel.h"
#include "t4r_internal.h"
#include "../../include/t4r_hip.h"
#include <atomic>

// k-tile depth of the fp32 form: 16.  BK = 32 (16 MFMAs per barrier) won isolated long-K launches (square 111 ->
// 115 TF, wgrads 72 -> 80, head dX 91 -> 96; tools/gemm_bench.py) but lost on the K = 128
// contractions (logits 85 -> 76 TF) and, selected per launch by K, made the whole training step
// slower (6.31 vs 6.23 ms, same box): the softmax-gradient variants paid for the doubled staging
// registers.  It was instantiated behind a switch until the forms were counted.  The depth itself is
// kBkF32 (gemm_kernel.h, beside kBkHalf = 32 of the half forms).

template <int BM, int BN, bool TA, bool TB, int FEAT>
static int launch_feat(const GemmParams& p, int batch, hipStream_t stream) {
    if (p.vecA && p.vecB) return launch_vec<BM, BN, kBkF32, TA, TB, FEAT, true>(p, batch, stream);
    return launch_vec<BM, BN, kBkF32, TA, TB, FEAT, false>(p, batch, stream);
}

// the 64 x 64 fp32 forms: the A-operand transform or epilogue of the launch picks FEAT.  The three layout errors are guards kept
// on purpose: today's callers pass transB = 0 with the softmax-gradient operand and NT, splitk 1 with the rank and collect
// epilogues, so none of them fires, but the other layouts of this template need some branch, and a plain product in its place
// would be a silent wrong answer.
template <bool TA, bool TB>
static int launch_cfg(const GemmParams& p, int batch, hipStream_t stream) {
    if (p.sg_lse) {
        if (!TB) return launch_feat<64, 64, TA, false, 1>(p, batch, stream);
        t4r_set_error("gemm: softmax-grad operand needs transB = 0");
        return -1;
    }
    if (p.rk_thr) {
        if (!TA && TB && p.splitk == 1) return launch_feat<64, 64, false, true, 4>(p, batch, stream);
        t4r_set_error("gemm: the rank epilogue needs the NT layout without split-K");
        return -1;
    }
    if (p.tk_thr) {
        if (!TA && TB && p.splitk == 1 && p.tk_filtered)
            return p.tk_noisy ? launch_feat<64, 64, false, true, 56>(p, batch, stream)
                              : launch_feat<64, 64, false, true, 40>(p, batch, stream);
        if (!TA && TB && p.splitk == 1)
            return p.tk_noisy ? launch_feat<64, 64, false, true, 24>(p, batch, stream)
                              : launch_feat<64, 64, false, true, 8>(p, batch, stream);
        t4r_set_error("gemm: the top-k collect epilogue needs the NT layout without split-K");
        return -1;
    }
    if (p.drop.p > 0.f && (p.epilogue == EPI_BIAS_GELU || p.epilogue == EPI_BIAS_RESID))
        return launch_feat<64, 64, TA, TB, 2>(p, batch, stream);
    return launch_feat<64, 64, TA, TB, 0>(p, batch, stream);
}

// ---- precision of the contraction (process-wide; the backward runs on autograd's thread, so not thread-local)
//   0 fp32 matrix cores (the reference's own arithmetic)
//   1 fp32-accurate on the bf16 matrix cores (exact 3-way split, six products) wherever the operands allow it
//   2 / 3 mixed precision, bf16 / fp16 operands, fp32 accumulation (the reference's AMP: trainer.py:363-367)
//   4 auto (default): fp32 accuracy, the split form on the shapes where it measured faster (see auto_split)
static std::atomic<int> g_prec{-1};
// 1 in an experiment build (-DT4R_EXPERIMENTAL): the host side reads its A/B switches only then (transformers4rec_amd/_lib.py: exp_env)
extern "C" int t4r_experimental_build(void) {
#ifdef T4R_EXPERIMENTAL
    return 1;
#else
    return 0;
#endif
}
extern "C" void t4r_set_precision(int mode) { g_prec.store(mode < 0 || mode > 4 ? 0 : mode); }
extern "C" int t4r_get_precision(void) {
    int m = g_prec.load();
    if (m < 0) {
        const char* e = getenv("T4R_GEMM_PREC");
        m = e ? atoi(e) : 4;        // default: auto (fp32 accuracy; the split form where it is faster)
        if (m < 0 || m > 4) m = 4;
        g_prec.store(m);
    }
    return m;
}

// shapes on which the split form beat the fp32 matrix cores (tools/gemm_bench.py --prec, profiles/r02_*)
constexpr double kAutoSplitMinFlop = 2e9;
static double gemm_flop(const GemmParams& p) { return 2.0 * p.M * p.N * (double)p.K; }
static bool auto_split(const GemmParams& p) { return gemm_flop(p) >= kAutoSplitMinFlop; }

// ---------------------------------------------------------------- deterministic split-K (two stages)
// Split-K launches normally add their partial tiles into C with fp32 atomics: run-to-run non-deterministic, and every
// split of a tile finishes at the same time and hits the same addresses (same-address atomics serialise at the memory
// side: a 128 x 128-tile experiment, tools/wgrad_planes_experiment.hip, lost 10-20 of 33-43 us to them).  A launch that
// is handed a SINK (t4r_internal.h: SplitKSink in GemmOpts; the XLNet layer backward keeps one on its stack over a slice
// of its scratch and passes it to its weight-gradient products, t4r_gemm_wgrad_f32 below over the caller's workspace)
// stores its partial tiles there instead and registers a job, if it accumulates; ONE launch
// (t4r_splitk_sink_flush) then adds the partials of every job in split order:  C += ((p0 + p1) + p2) + ...
// The second stages of the layer's column reductions (bias / LayerNorm / attention-bias gradients) ride in the same
// launch (t4r_splitk_sink_add_reduce, through the layer's ReduceCtx): one reduction launch per layer backward instead of
// four small ones + atomics.  The sink is an argument everywhere: a launch that was not given one never finds one.
// Measured in the step at BASELINE configs[1] (single stream, rocprofv3): FF weight gradients 33.8 -> 32.3 us, the
// D x D ones 24.2 -> 20.5 us, the reduction 11 us per layer: 560 -> 549 us per step.  The point is the fixed order:
// the body's parameter gradients are now bit-reproducible run to run (tests/test_kernels_gpu.py).

// workgroup = 16 float4 columns x 16 split groups; group g adds splits g, g + 16, ... in order (four loads in flight per
// thread: a job with 256 partial rows and 32 columns is ONE workgroup, its time is its dependent load chain), then the
// groups are added in order
__device__ __forceinline__ void add4(float4& a, const float4 v) { a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
__global__ __launch_bounds__(256) void splitk_reduce_kernel(SplitKJobs jobs) {
    __shared__ float4 sm[16][16];
    int ji = 0;
    while (ji + 1 < jobs.n && (int)blockIdx.x >= jobs.blk_end[ji]) ++ji;
    const SplitKJob job = jobs.j[ji];
    const int b = blockIdx.x - (ji ? jobs.blk_end[ji - 1] : 0);
    const int c = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int i = b * 16 + c;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < job.n4) {
        const float4* p = reinterpret_cast<const float4*>(job.part) + i;
        int s = g;
        for (; s + 48 < job.splits; s += 64) {
            const float4 v0 = p[(long)s * job.stride4], v1 = p[(long)(s + 16) * job.stride4];
            const float4 v2 = p[(long)(s + 32) * job.stride4], v3 = p[(long)(s + 48) * job.stride4];
            add4(acc, v0); add4(acc, v1); add4(acc, v2); add4(acc, v3);
        }
        for (; s < job.splits; s += 16) add4(acc, p[(long)s * job.stride4]);
    }
    sm[g][c] = acc;
    __syncthreads();
    if (g == 0 && i < job.n4) {
#pragma unroll
        for (int r = 1; r < 16; ++r) add4(acc, sm[r][c]);
        float4* o = reinterpret_cast<float4*>(job.out) + i;
        if (job.accumulate) add4(acc, *o);
        *o = acc;
    }
}

int t4r_splitk_sink_flush(SplitKSink& sink, hipStream_t st) {
    SplitKJobs& J = sink.jobs;
    if (J.n > 0) {
        int blocks = 0;
        for (int i = 0; i < J.n; ++i) { blocks += (J.j[i].n4 + 15) / 16; J.blk_end[i] = blocks; }
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, st, J);
        T4R_LAUNCH_CHECK();
    }
    J.n = 0;       // the partial buffers stay taken for the life of the sink: a later flush may run on another stream
    return 0;
}

// a split-K launch asks for room: returns the partial buffer (and registers the jobs) or null (-> atomics).  sink->bypassed
// counts the ELIGIBLE launches that got none (buffer too small, too many jobs): correct, but not bit-reproducible
static float* splitk_sink_take(SplitKSink* sink, const GemmParams& p, int batch) {
    if (!sink || !p.accumulate || p.epilogue != EPI_NONE || p.sg_lse || p.rk_thr || p.tk_thr) return nullptr;
    SplitKSink& k = *sink;
    const long n = (long)p.M * p.ldc;                       // one partial = C's [M][ldc] image (dense outputs: ldc == N)
    if (p.ldc != p.N || n % 4 || ((uintptr_t)p.C & 15) || (p.sC % 4)) return nullptr;        // not a shape the sink takes
    if (k.jobs.n + batch > kMaxSplitKJobs) { ++k.bypassed; return nullptr; }
    const long need = n * p.splitk * batch;
    if (k.used + need > k.cap || n / 4 > 0x7fffffffL) { ++k.bypassed; return nullptr; }
    float* part = k.ws + k.used;
    k.used += need;
    for (int b = 0; b < batch; ++b)
        k.jobs.j[k.jobs.n++] = SplitKJob{part + (long)b * p.splitk * n, p.C + b * p.sC, (int)(n / 4), p.splitk, n / 4, 1};
    return part;
}
// the second stage of a column reduction (elementwise.hip: t4r_reduce_partials_launch, out_s[i] (+)= sum_b part[b * n + off_s + i])
// joins the sink's launch: false -> the caller launches its own kernel
bool t4r_splitk_sink_add_reduce(SplitKSink& k, const float* part, int nblocks, int n, float* const* outs, const int* lens,
                                const int* accs, int n_seg) {
    if (nblocks <= 0 || (n & 3) || ((uintptr_t)part & 15)) return false;
    int live = 0;
    for (int s = 0; s < n_seg; ++s) {
        if (lens[s] & 3) return false;
        // only sums ACCUMULATED into their output are deferred (parameter gradients, read after the layer); an overwriting
        // one is an intermediate of the layer (d k_r with a shared k_r feeds the r weight gradient) and runs at once
        if (outs[s] && lens[s] > 0) { if (((uintptr_t)outs[s] & 15) || !accs[s]) return false; ++live; }
    }
    if (k.jobs.n + live > kMaxSplitKJobs) return false;
    int off = 0;
    for (int s = 0; s < n_seg; ++s) {
        if (outs[s] && lens[s] > 0) k.jobs.j[k.jobs.n++] = SplitKJob{part + off, outs[s], lens[s] / 4, nblocks, n / 4, accs[s]};
        off += lens[s];
    }
    return true;
}

// Split-K.  Enough workgroups to fill 256 CUs x 8 (the k-loop of one workgroup hides latency only
// through other resident workgroups), but at least ~20 k-tiles each so that the atomics of
// the epilogue stay a small part.  Measured (tools/gemm_bench.py): head dX 2765x128x100001
// 1076 us at 1024 workgroups, 786 us at 4096; wgrad 128x512x20480 best at 64 splits.
constexpr long kSplitTargetBlocks = 4096, kSplitMinTiles = 20;
constexpr int kSplitMax = 256;
// what ONE product with splitk = -1 can need in a sink: never more splits than this (the k-tile is at least kBkF32 deep)
extern "C" long t4r_gemm_wgrad_ws_floats(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return (long)M * N * min((long)kSplitMax, K / (kSplitMinTiles * kBkF32) + 1);
}

// opt (t4r_internal.h: GemmOpts): the operand maxima of this launch and the sink of its split-K partial tiles (null: none)
// force_fp32 (the fused top-k head only: t4r_gemm_fp32_nt_launch / t4r_gemm_topk_collect_launch): this launch runs form 0
// whatever the process-wide mode says, so that its outputs carry the bits of the materialised fp32 scores
template <bool TA, bool TB>
static int launch_layout(GemmParams& p, int batch, int splitk_req, hipStream_t stream, const GemmOpts& opt, bool force_fp32) {
    auto launch_precision = [&]() { return force_fp32 ? 0 : t4r_get_precision(); };
    const GemmAmax* amax = opt.amax;
    const float* amax_a = amax ? amax->a : nullptr;
    const float* amax_b = amax ? amax->b : nullptr;
    const int amax_n = amax ? amax->na : 0, amax_nb = amax ? amax->nb : 0;
    p.amaxA = p.amaxB = nullptr; p.n_amax = p.n_amax_b = 0;
#ifdef T4R_EXPERIMENTAL
    // long-K weight gradients that were handed a split-K sink (the XLNet layer backward): the K-streaming kernel (wgrad_stream.hip)
    if (TA && !TB && splitk_req < 0 && opt.sink && t4r_wgrad_stream_ok(p)) {
        int splits = 1, kper = 0;
        t4r_wgrad_stream_plan(p.K, &splits, &kper);
        p.splitk = splits;
        float* part = splitk_sink_take(opt.sink, p, batch);
        if (part) return t4r_wgrad_stream_launch(p, batch, kper, part, stream);
        p.splitk = 1;
    }
    if (TA && !TB && splitk_req < 0 && opt.sink && amax_a && amax_b) {
        p.amaxA = amax_a; p.amaxB = amax_b; p.n_amax = amax_n; p.n_amax_b = amax_nb;
        if (t4r_wgrad_units_ok(p)) {
            int splits = 1, kper = 0;
            t4r_wgrad_units_plan(p.K, &splits, &kper);
            p.splitk = splits;
            float* part = splitk_sink_take(opt.sink, p, batch);
            if (part) return t4r_wgrad_units_launch(p, batch, kper, part, stream);
            p.splitk = 1;
        }
        p.amaxA = p.amaxB = nullptr; p.n_amax = p.n_amax_b = 0;
    }
#endif
    // tokens x small weight in an fp32-accurate mode: the token-stationary kernel (operands cut once, tok_gemm.hip)
    if (!TA && (splitk_req == 0 || splitk_req == 1)) {
        const int mode = launch_precision();
        if (mode == 4 || mode == 1) {
            p.splitk = 1;
            const int rc = t4r_tok_gemm_try(p, batch, TA, TB, stream);
            if (rc) return rc < 0 ? rc : 0;
        }
    }
    // Tile.  Measured on MI355X (tools/gemm_bench.py, profiles/r01_b_gemm_tile_sweep.txt): on the layer shapes
    // and the head's backward products the 64x64x16 tile (7-8 waves/SIMD resident) beats the 128-wide
    // tiles -- latency- not LDS-bound, more workgroups in flight win (head dW 47 -> 79 TF/s).  Three forms
    // take a larger one, each chosen by shape below (DESIGN.md 4.1.2 lists every form and what selects it).
    int bm = 64, bn = 64;
    const bool feat = p.sg_lse || (p.drop.p > 0.f && (p.epilogue == EPI_BIAS_GELU || p.epilogue == EPI_BIAS_RESID));
    // the vocabulary-wide logits product (end-of-round pipeline): per output the workgroup pulls half
    // as much of X and W through L2 with a 128 x 128 tile, 759 vs 797 us stand-alone at C2
    const bool logits_shape = !TA && TB && p.M >= 1024 && p.N >= 32768 && !p.sg_lse && !p.rk_thr && !p.tk_thr && p.epilogue == EPI_NONE;
    // precision of this launch: the half-precision variants need 16-byte loadable operands; the rank epilogue
    // (exact ranks of the evaluation head) always stays on the fp32 matrix cores
    int prec = launch_precision();
    if (prec == 4) prec = auto_split(p) ? 1 : 0;
    if (prec && (!(p.vecA && p.vecB) || p.rk_thr || p.tk_thr)) prec = 0;
    if (prec && p.sg_lse && TB) prec = 0;
    if (prec == 1 && amax_a && amax_b && !feat && p.epilogue == EPI_NONE) {
        prec = 4; p.amaxA = amax_a; p.amaxB = amax_b; p.n_amax = amax_n; p.n_amax_b = amax_nb;       // always 64 x 64
    } else if (prec == 1) {
        // measured (profiles/r02_b_gemm_prec_bench.txt): the 128 x 64 tile (half the A-operand LDS reads per MFMA)
        // wins the large plain products (C5 body 2459 -> 2233 us, square 4096 1051 -> 944 us, logits 700 -> 693 us)
        // and loses or ties below ~20 GFLOP.  Never 128 x 128: the three-plane images of such a tile take 101 KB of LDS
        if (!feat && p.M >= 1024 && p.N >= 512 && gemm_flop(p) >= 2e10) bm = 128;
    } else if (logits_shape) {          // fp32 and the one-plane precisions
        bm = bn = 128;
    }
    // Split-K (the rule's constants: above launch_layout)
    const int kt = (p.K + (prec ? kBkHalf : kBkF32) - 1) / (prec ? kBkHalf : kBkF32);
    int splitk = splitk_req;
    if (splitk_req == 0) {  // auto: only when the caller allows atomics (accumulating outputs)
        splitk = 1;
    } else if (splitk_req < 0) {
        const long blocks = (long)((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn) * batch;
        splitk = (int)max(1L, min((long)kt / kSplitMinTiles, kSplitTargetBlocks / max(1L, blocks)));
        splitk = min(splitk, kSplitMax);
    }
    p.splitk = max(1, splitk);
    p.part = nullptr;
    if (p.splitk > 1) {
        // every split owns at least one k-tile (a partial tile must be written by its split)
        const int kt_per = (kt + p.splitk - 1) / p.splitk;
        p.splitk = (kt + kt_per - 1) / kt_per;
        if (p.splitk > 1) p.part = splitk_sink_take(opt.sink, p, batch);
    }
    p.xcd_order = 1;        // XCD-aware tile order (gemm_kernel.h); the kernel keeps the test of it
    if (p.splitk > 1) {
        if (p.epilogue != EPI_NONE) { t4r_set_error("gemm: split-K needs epilogue NONE"); return -1; }
        if (!p.accumulate && !p.part) {  // atomics accumulate: start from zero unless the caller accumulates
            for (int b = 0; b < batch; ++b)
                (void)hipMemset2DAsync(p.C + b * p.sC, p.ldc * sizeof(float), 0, p.N * sizeof(float), p.M, stream);
        }
    }
    if (prec) return t4r_gemm_half_dispatch(p, batch, TA, TB, bm, bn, prec, stream);
    if constexpr (!TA && TB) {
        if (bm == 128) return launch_feat<128, 128, false, true, 0>(p, batch, stream);
    }
    return launch_cfg<TA, TB>(p, batch, stream);
}

struct SoftmaxGradA { const float* lse; const long* labels; const float* gout; int rows, V; float smooth; int yoff; };
struct RankEpi { const float* thr; const long* label; int* count; };
struct TopkEpi { const float* thr; long thr_ld; int* count; float* val; int* idx; int cap; const GumbelCfg* noise; const ItkFilter* filt; };

// sg: the softmax-gradient A operand (t4r_gemm_softmax_grad_launch); rank: the rank epilogue (t4r_rank_of_target_f32);
// topk / force_fp32: the two products of the fused top-k head (end of this file); null / false everywhere else
static int gemm_launch_impl(hipStream_t stream, int transA, int transB, int M, int N, int K, float alpha,
                            const float* A, long lda, const float* B, long ldb, float* C, long ldc,
                            const float* bias, int epilogue, float* aux, long ldaux, int splitk,
                            int accumulate, int batch, long sA, long sB, long sC, const DropCfg* drop,
                            const SoftmaxGradA* sg, const RankEpi* rank, const TopkEpi* topk, bool force_fp32,
                            const GemmOpts& opt = GemmOpts()) {
    if (M <= 0 || N <= 0) return 0;
    T4R_CHECK_ARG(K > 0 && A && B && C && batch >= 1, "gemm: bad arguments");
    GemmParams p;
    p.M = M; p.N = N; p.K = K;
    p.A = A; p.lda = lda; p.B = B; p.ldb = ldb; p.C = C; p.ldc = ldc;
    p.bias = bias; p.aux = aux; p.ldaux = ldaux; p.alpha = alpha; p.epilogue = epilogue;
    p.accumulate = accumulate; p.sA = sA; p.sB = sB; p.sC = sC;
    p.vecA = ((uintptr_t)A % 16 == 0) && (lda % 4 == 0) && (sA % 4 == 0);
    p.vecB = ((uintptr_t)B % 16 == 0) && (ldb % 4 == 0) && (sB % 4 == 0);
    p.splitk = 1;
    p.part = nullptr;
    p.drop = drop ? *drop : make_drop(0.f, 0, 0);
    p.sg_lse = nullptr; p.sg_labels = nullptr; p.sg_gout = nullptr; p.sg_rows = 1; p.sg_V = 1; p.sg_smooth = 0.f; p.sg_yoff = 0;
    p.rk_thr = nullptr; p.rk_label = nullptr; p.rk_count = nullptr;
    if (rank) { p.rk_thr = rank->thr; p.rk_label = rank->label; p.rk_count = rank->count; }
    p.tk_thr = nullptr; p.tk_thr_ld = 0; p.tk_count = nullptr; p.tk_val = nullptr; p.tk_idx = nullptr; p.tk_cap = 0;
    p.tk_noisy = 0; p.tk_noise = GumbelCfg{0, 0, 0};
    p.tk_filtered = 0; p.tk_filt = ItkFilter{nullptr, nullptr, 0, 0};
    if (topk) {
        p.tk_thr = topk->thr; p.tk_thr_ld = topk->thr_ld; p.tk_count = topk->count;
        p.tk_val = topk->val; p.tk_idx = topk->idx; p.tk_cap = topk->cap;
        if (topk->noise) { p.tk_noisy = 1; p.tk_noise = *topk->noise; }
        if (topk->filt) { p.tk_filtered = 1; p.tk_filt = *topk->filt; }
    }
    if (sg) {
        p.sg_lse = sg->lse; p.sg_labels = sg->labels; p.sg_gout = sg->gout;
        p.sg_rows = sg->rows; p.sg_V = sg->V; p.sg_smooth = sg->smooth; p.sg_yoff = sg->yoff;
    }
    if (transA) {
        if (transB) return launch_layout<true, true>(p, batch, splitk, stream, opt, force_fp32);
        return launch_layout<true, false>(p, batch, splitk, stream, opt, force_fp32);
    }
    if (transB) return launch_layout<false, true>(p, batch, splitk, stream, opt, force_fp32);
    return launch_layout<false, false>(p, batch, splitk, stream, opt, force_fp32);
}

// Internal C++ entry used by the composite (layer / head) launchers.
int t4r_gemm_launch(hipStream_t stream, int transA, int transB, int M, int N, int K, float alpha,
                    const float* A, long lda, const float* B, long ldb, float* C, long ldc,
                    const float* bias, int epilogue, float* aux, long ldaux, int splitk,
                    int accumulate, int batch, long sA, long sB, long sC, const DropCfg* drop, GemmOpts opt) {
    return gemm_launch_impl(stream, transA, transB, M, N, K, alpha, A, lda, B, ldb, C, ldc, bias, epilogue, aux, ldaux, splitk,
                            accumulate, batch, sA, sB, sC, drop, nullptr, nullptr, nullptr, false, opt);
}

extern "C" int t4r_gemm_f32(void* stream, int transA, int transB, int M, int N, int K, float alpha,
                            const float* A, long lda, const float* B, long ldb, float* C, long ldc,
                            const float* bias, int epilogue, float* aux, long ldaux, int splitk,
                            int accumulate, int batch, long strideA, long strideB, long strideC,
                            float drop_p, unsigned long long seed, unsigned long long ctr_hi) {
    T4R_CHECK_ARG(epilogue != EPI_BIAS_RESID || aux, "gemm: EPI_BIAS_RESID needs the residual in aux");
    const DropCfg dc = make_drop(drop_p, seed, ctr_hi);
    return t4r_gemm_launch((hipStream_t)stream, transA, transB, M, N, K, alpha, A, lda, B, ldb, C,
                           ldc, bias, epilogue, aux, ldaux, splitk, accumulate, batch, strideA,
                           strideB, strideC, drop_p > 0.f ? &dc : nullptr);
}

// include/t4r_hip.h.  A weight gradient outside the layer (the input block's projection, features.py: once the one
// order-dependent sum of a BASELINE configs[2] step): the sink lives on this stack for one product and its reduction.
// ws may be null where the size query returns M * N (one split: nothing is parked).
extern "C" int t4r_gemm_wgrad_f32(void* stream, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
                                  float* C, float* ws, long ws_floats, int* bypassed) {
    if (bypassed) *bypassed = 0;
    SplitKSink sink(ws, ws_floats);
    const int rc = t4r_gemm_launch((hipStream_t)stream, 1, 0, M, N, K, 1.f, A, lda, B, ldb, C, N, nullptr, EPI_NONE, nullptr, 0,
                                   -1, 1, 1, 0, 0, 0, nullptr, GemmOpts{nullptr, &sink});
    if (rc != 0) return rc;
    if (bypassed) *bypassed = sink.bypassed != 0;
    return t4r_splitk_sink_flush(sink, (hipStream_t)stream);
}

// Head backward contractions with CrossEntropyLoss' backward fused into the A operand:
//   transA = 0:  C[N_rows, N] (+)= alpha * dlogits[N_rows, V] @ B[V, N]          (d X = dlogits @ W)
//   transA = 1:  C[V, N]     (+)= alpha * dlogits[N_rows, V]^T @ B[N_rows, N]    (d W = dlogits^T @ X)
// where dlogits = (*grad_out / N_rows) * (softmax(logits) - target) is formed from `logits`,
// `lse` and `labels` while the tile is staged.  Replaces model/prediction_task.py:446 (loss
// backward through CrossEntropyLoss) + the autograd of :664.
// logits holds the columns [yoff, yoff + Vc) of the full [n_rows, V] logits (Vc = V, yoff = 0: all of them);
// the label-smoothing term eps / V and the mean 1 / n_rows refer to the full problem.
int t4r_gemm_softmax_grad_launch(hipStream_t stream, int transA, int n_rows, int Vc, int V, int yoff, int N,
                                 float alpha, const float* logits, long ld_logits, const float* lse,
                                 const long* labels, const float* grad_out, float label_smoothing, const float* B,
                                 long ldb, float* C, long ldc, int splitk, int accumulate) {
    T4R_CHECK_ARG(lse && labels && logits, "gemm_softmax_grad: null operand");
    const SoftmaxGradA sg{lse, labels, grad_out, n_rows, V, label_smoothing, yoff};
    const int M = transA ? Vc : n_rows, K = transA ? n_rows : Vc;
    return gemm_launch_impl(stream, transA, 0, M, N, K, alpha, logits, ld_logits, B, ldb, C, ldc, nullptr, EPI_NONE, nullptr, 0,
                            splitk, accumulate, 1, 0, 0, 0, nullptr, &sg, nullptr, nullptr, false);
}

extern "C" int t4r_gemm_softmax_grad_f32(void* stream, int transA, int n_rows, int V, int N, float alpha,
                                         const float* logits, long ld_logits, const float* lse,
                                         const long* labels, const float* grad_out, float label_smoothing,
                                         const float* B, long ldb, float* C, long ldc, int splitk,
                                         int accumulate) {
    return t4r_gemm_softmax_grad_launch((hipStream_t)stream, transA, n_rows, V, V, 0, N, alpha, logits, ld_logits,
                                        lse, labels, grad_out, label_smoothing, B, ldb, C, ldc, splitk, accumulate);
}

// Fused eval head: rank of the target item among alpha * X @ W^T without materialising
// the [n_rows, V] scores.  target_score[row] must be the row's own score of its label column as THIS
// kernel computes it (run t4r_gemm_f32 on the gathered label rows of W and take the diagonal: an
// output element's bits do not depend on its tile position).  rank[row] (int32) is overwritten with
// #{v : score_v > target or (score_v == target and v < label)}: Recall@k = rank < k,
// NDCG@k = rank < k ? 1 / log2(rank + 2) : 0  (ranking_metric.py:107-147, 242-280 with one relevant item).
extern "C" int t4r_rank_of_target_f32(void* stream, int n_rows, int V, int D, float alpha, const float* X,
                                      long ldx, const float* W, long ldw, const float* target_score,
                                      const long* labels, int* rank) {
    if (n_rows == 0) return 0;
    T4R_CHECK_ARG(target_score && labels && rank, "rank_of_target: null pointer");
    if (hipMemsetAsync(rank, 0, sizeof(int) * (size_t)n_rows, (hipStream_t)stream) != hipSuccess) {
        t4r_set_error("rank_of_target: memset failed");
        return -1;
    }
    const RankEpi re{target_score, labels, rank};
    // C is never written by the rank epilogue; a non-null dummy keeps the argument check happy
    return gemm_launch_impl((hipStream_t)stream, 0, 1, n_rows, V, D, alpha, X, ldx, W, ldw, reinterpret_cast<float*>(rank), V,
                            nullptr, EPI_NONE, nullptr, 0, 1, 0, 1, 0, 0, 0, nullptr, nullptr, &re, nullptr, false);
}

// ---- the two products of the fused top-k inference head (csrc/item_topk.hip), both form 0 whatever the process-wide mode:
// C[M, N] = alpha * A[M, K] @ B[N, K]^T with the ordinary epilogue ...
int t4r_gemm_fp32_nt_launch(hipStream_t stream, int M, int N, int K, float alpha, const float* A, long lda,
                            const float* B, long ldb, float* C, long ldc) {
    return gemm_launch_impl(stream, 0, 1, M, N, K, alpha, A, lda, B, ldb, C, ldc, nullptr, EPI_NONE, nullptr, 0, 1, 0, 1, 0, 0,
                            0, nullptr, nullptr, nullptr, nullptr, true);
}
// ... and the same product with the collect epilogue: no C; (score, item) of every score >= thr[row * thr_ld] goes to the
// row's candidate list (GemmParams::tk_*).  count[n_rows] must be zero on entry.
// noise (null: none): the sampling head's collect, v + g(row0 + row, col) before the compare (gumbel_noise.h).
int t4r_gemm_topk_collect_launch(hipStream_t stream, int n_rows, int V, int D, float alpha, const float* X, long ldx,
                                 const float* W, long ldw, const float* thr, long thr_ld, int* count, float* cand_val,
                                 int* cand_idx, int cap, const GumbelCfg* noise) {
    const TopkEpi te{thr, thr_ld, count, cand_val, cand_idx, cap, noise, nullptr};
    // C is never written by the collect epilogue; a non-null dummy keeps the argument check happy
    return gemm_launch_impl(stream, 0, 1, n_rows, V, D, alpha, X, ldx, W, ldw, cand_val, V, nullptr, EPI_NONE, nullptr, 0, 1, 0,
                            1, 0, 0, 0, nullptr, nullptr, nullptr, &te, true);
}
// ... and under an item filter (item_filter.h): only allowed items are appended
int t4r_gemm_topk_collect_filtered_launch(hipStream_t stream, int n_rows, int V, int D, float alpha, const float* X, long ldx,
                                          const float* W, long ldw, const float* thr, long thr_ld, int* count, float* cand_val,
                                          int* cand_idx, int cap, const GumbelCfg* noise, const ItkFilter* filt) {
    const TopkEpi te{thr, thr_ld, count, cand_val, cand_idx, cap, noise, filt};
    return gemm_launch_impl(stream, 0, 1, n_rows, V, D, alpha, X, ldx, W, ldw, cand_val, V, nullptr, EPI_NONE, nullptr, 0, 1, 0,
                            1, 0, 0, 0, nullptr, nullptr, nullptr, &te, true);
}
