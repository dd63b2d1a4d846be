// Inference head over a half-precision SERVING IMAGE of the item table (gfx950 only).
//
// Replaces, for a served model, the last-item scores + torch.topk of the reference
// (transformers4rec/torch/model/prediction_task.py:452-470, :664) as they run under fp16=True / bf16=True, i.e. under autocast
// (transformers4rec/torch/trainer.py:363-367): ONE 16-bit matrix-core product per multiply, fp32 accumulation.
//
//   score[n, v] = alpha * acc[n, v],   acc[n, v] = sum_d x16[n, d] * img[v, d]   (fp32 accumulation on the matrix cores)
//
// x16 = round-to-nearest-even(x) in the image's dtype, img = the packed table.  No operand scaling: autocast's semantics and its
// range (fp16 overflows above 65 504).  Products of two fp16 / two bf16 numbers are exact in fp32, so the only rounding after the
// operands is the accumulation.
//
// Kernels
//   itk16_round_rows_kernel   fp32 [R, D] (any pitch) -> 16-bit [R, ldp], RNE, pad columns D..ldp-1 zero.  ldp = D rounded up to the
//                             k step (16 elements = 32 bytes), so rows are 16-byte aligned and the k loop has no edge.  It is the
//                             PACK of the table (once per table) and the prologue that rounds x (once per call, <= 1 MB).
//   itk16_kernel<DT, EPI>     item-tile-stationary product.  A workgroup (4 waves) loads 64 image rows with 16-byte loads into LDS
//                             -- row pitch 2 ldp + 16 bytes: an odd number of 16-byte slots, so the 16 rows a ds_read_b128 lane
//                             group touches fall on 16 different slots of the 256-byte bank row (conflict free); 65 KB at D = 512,
//                             two workgroups per CU -- and walks the rows of x16 against it: a wave takes 32 rows x 64 items
//                             (two v_mfma_f32_32x32x16_f16 / _bf16 accumulators), its A fragments come straight from x16 (L2 / L1:
//                             x16 is the operand that is re-read), its B fragments from the LDS image.  Every image row is loaded by
//                             exactly one workgroup, once: the image comes from HBM once per launch.
//                             EPI 0 stores alpha * acc to C (fp32); EPI 1 is the top-k COLLECT epilogue of gemm_kernel.h (FEAT bit 3),
//                             the same function (itk_collect, item_topk_collect.h): compare with the row's threshold, one ballot
//                             per 32-lane half (a half holds 32 consecutive items of one row), one returning slot atomic by the
//                             half's first lane, hits stored at base + prefix.
//                             `stride` > 1 scores the strided sample of step 1 in place (item i of the launch is image row
//                             i * stride): no gathered copy of the sample.
//                             EPI 2 is EPI 1 over fp32(alpha * acc + g(row, item)): the collect pass of the sampling head
//                             (t4r_item_sample_h16; gumbel_noise.h, ItkNoisyHead in item_topk_plan.h).
//                             EPI 3 / 4 are EPI 1 / 2 under an item filter (include/t4r_hip_filter.h, item_filter.h): the allow
//                             bit is folded into the compare, the row's exclusion list is searched behind a non-empty ballot.
//                             The tile load and the k loop live in item_h16_tile.h, shared with item_eval_h16.hip, as do the
//                             image's argument contract and the dtype dispatch.
//   select / threshold top-k  itk_select_kernel (item_topk.hip) and t4r_topk, unchanged; the plan and the four-step driver
//                             (itk_run) are item_topk_plan.h's, shared with item_topk.hip: this file's part is Itk16Head.
//
// Bits.  One element is computed by ONE instruction sequence whatever launch, tile or row block it sits in: k runs 0, 16, 32, ...
// to ldp in every launch, each step one MFMA into the same accumulator, then one multiplication by alpha.  The sampled thresholds,
// the collected candidates and the materialised scores of the same (row, item) are therefore the same bits, which is what makes
// "fused == materialised" exact; rows that overflow their list take the materialised path in this same arithmetic.
//
// Widths: 1 <= D <= 512 (t4r_item_topk_h16_supported).  Wider tables are refused with a message: the 64-row LDS image of a
// workgroup would leave one workgroup per CU, and no model of this project is wider.
//
// fp16 subnormals: observed on MI355X (tests/test_item_topk_h16_gpu.py::test_fp16_subnormal_operands, 130 940 subnormal table
// entries at 64 x 4099 x 128): the matrix cores HONOUR subnormal fp16 operands -- largest error 9.6e-6, inside the plain
// accumulation bound at every element, against 5.0e-4 to a reference with those entries flushed.  The contract tests still allow
// either behaviour for entries below 2^-14.
#include "item_h16_tile.h"
#include "item_topk_collect.h"
#include "item_topk_plan.h"

namespace {

// one 16-byte chunk (8 elements) per thread
template <int DT>
__global__ __launch_bounds__(256) void itk16_round_rows_kernel(const float* __restrict__ src, long lds_, long rows, int D,
                                                                uint16_t* __restrict__ dst, long ldp, int chunks, int vec) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * chunks) return;
    const long r = i / chunks;
    const int c0 = (int)(i % chunks) * 8;
    const float* s = src + r * lds_ + c0;
    float v[8];
    if (vec && c0 + 8 <= D) {
        const float4 a = *reinterpret_cast<const float4*>(s), b = *reinterpret_cast<const float4*>(s + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = c0 + e < D ? s[e] : 0.f;
    }
    uint4 o;
    o.x = round16<DT>(v[0]) | (round16<DT>(v[1]) << 16);
    o.y = round16<DT>(v[2]) | (round16<DT>(v[3]) << 16);
    o.z = round16<DT>(v[4]) | (round16<DT>(v[5]) << 16);
    o.w = round16<DT>(v[6]) | (round16<DT>(v[7]) << 16);
    *reinterpret_cast<uint4*>(dst + r * ldp + c0) = o;
}

struct Itk16Params {
    int n_rows, n_items, ldp;       // ldp: k extent (multiple of 16) = pitch of x16
    const uint16_t* x16;            // [n_rows, ldp]
    const uint16_t* img; long ldi;  // item i of the launch = image row i * stride
    int stride;
    float alpha;
    float* C; long ldc;             // EPI 0
    const float* thr; long thr_ld;  // EPI 1: as GemmParams::tk_*
    int* count;
    float* cand_val;
    int* cand_idx;
    int cap;
    GumbelCfg noise;                // EPI 2: EPI 1 over fp32(v + g(row, item)) (gumbel_noise.h)
    ItkFilter filt;                 // EPI 3 / 4: EPI 1 / 2 over the allowed items only (item_filter.h)
};

template <int DT, int EPI>
__global__ __launch_bounds__(256) void itk16_kernel(Itk16Params p) {
    extern __shared__ uint4 itk16_lds[];                    // [64][chunks + 1] 16-byte slots
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunks = p.ldp >> 3, pitch = chunks + 1;
    const long item0 = (long)blockIdx.x * ITK16_TILE;
    itk16_load_tile(itk16_lds, p.img, p.ldi, p.stride, item0, p.n_items, chunks, tid);
    __syncthreads();
    const int r = lane & 31, h = lane >> 5;
    const uint4* b0p = itk16_lds + r * pitch + h;           // items item0 + r and item0 + 32 + r; k-step s is slot 2 s + h
    const uint4* b1p = itk16_lds + (32 + r) * pitch + h;
    const int nk = p.ldp >> 4;                              // k-steps
    const float alpha = p.alpha;
    for (int rb = wave * 32; rb < p.n_rows; rb += 128) {    // wave-uniform
        // rows beyond n_rows read the last row (a legal address) and are masked in the epilogue
        const uint4* ap = reinterpret_cast<const uint4*>(p.x16 + (long)min(rb + r, p.n_rows - 1) * p.ldp) + h;
        float thr[16];
        if (EPI != 0) {
#pragma unroll
            for (int e = 0; e < 16; ++e)
                thr[e] = p.thr[(long)min(rb + itk16_acc_row(e, h), p.n_rows - 1) * p.thr_ld];
        }
        f32x16 acc[2];
        itk16_product<DT>(ap, b0p, b1p, nk, acc);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const long col = item0 + j * 32 + r;
            if (EPI >= 3) {
                // the collect pass runs at stride 1: col is the item.  A lane's column is fixed over the 16 elements and the 32
                // lanes of a half hold the 32 columns from item0 + 32 j: one allow word per lane and block, the half's.
                const bool ok = col < p.n_items && ((itk_allow_word(p.filt.allow_bits, item0 + j * 32) >> r) & 1u);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float g[4];
                    if (EPI == 4) gumbel_quad(p.noise, rb + itk16_acc_row(4 * q, h), (uint32_t)col, g);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int row = rb + itk16_acc_row(4 * q + e, h);
                        float v = alpha * acc[j][4 * q + e];
                        if (EPI == 4) v = gumbel_perturb(v, g[e]);
                        itk_collect_filtered(ok && row < p.n_rows && v >= thr[4 * q + e], v, (int)col, row, lane, p.count,
                                             p.cand_val, p.cand_idx, p.cap, p.filt);
                    }
                }
                continue;
            }
            if (EPI == 2) {
                // elements 4 q .. 4 q + 3 of a lane are four consecutive rows of its column: one Philox block
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float g[4];
                    gumbel_quad(p.noise, rb + itk16_acc_row(4 * q, h), (uint32_t)(col * p.stride), g);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int row = rb + itk16_acc_row(4 * q + e, h);
                        const float v = gumbel_perturb(alpha * acc[j][4 * q + e], g[e]);
                        itk_collect(col < p.n_items && row < p.n_rows && v >= thr[4 * q + e], v, (int)col, row, lane, p.count,
                                    p.cand_val, p.cand_idx, p.cap);
                    }
                }
                continue;
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = rb + itk16_acc_row(e, h);
                const float v = alpha * acc[j][e];
                if (EPI == 0) {
                    if (col < p.n_items && row < p.n_rows) p.C[(long)row * p.ldc + col] = v;
                } else {
                    itk_collect(col < p.n_items && row < p.n_rows && v >= thr[e], v, (int)col, row, lane, p.count, p.cand_val,
                                p.cand_idx, p.cap);
                }
            }
        }
    }
}

T4rLdsAttr g_lds_attr[2][5];

template <int DT, int EPI>
int launch_t(hipStream_t st, const Itk16Params& p) {
    const size_t smem = itk16_lds_bytes(p.ldp);
    const void* fn = (const void*)itk16_kernel<DT, EPI>;
    t4r_ensure_dynamic_lds(fn, smem, g_lds_attr[DT - 2][EPI]);
    const unsigned grid = (unsigned)(((long)p.n_items + ITK16_TILE - 1) / ITK16_TILE);
    hipLaunchKernelGGL((itk16_kernel<DT, EPI>), dim3(grid), dim3(256), smem, st, p);
    T4R_LAUNCH_CHECK();
    return 0;
}

int launch(hipStream_t st, int dtype, int epi, const Itk16Params& p) {
    return itk16_dispatch(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (epi >= 3) return epi == 4 ? launch_t<DT, 4>(st, p) : launch_t<DT, 3>(st, p);
        return epi == 2 ? launch_t<DT, 2>(st, p) : (epi ? launch_t<DT, 1>(st, p) : launch_t<DT, 0>(st, p));
    });
}

// the image on the 16-bit matrix cores: the head object of itk_run.  p holds what every launch of the call shares.
struct Itk16Head {
    int dtype;
    Itk16Params p;                  // n_rows, ldp, x16, img, ldi, alpha

    int sample(hipStream_t st, const Plan& pl, float* S) const {       // in place: item i of the launch is image row i * stride
        Itk16Params q = p;
        q.n_items = pl.M; q.stride = pl.stride; q.C = S; q.ldc = pl.ldS;
        return launch(st, dtype, 0, q);
    }
    int collect(hipStream_t st, const float* thr, long thr_ld, int* count, float* cand_val, int* cand_idx, int cap,
                const GumbelCfg* noise = nullptr, const ItkFilter* filt = nullptr) const {
        Itk16Params q = p;
        q.thr = thr; q.thr_ld = thr_ld; q.count = count; q.cand_val = cand_val; q.cand_idx = cand_idx; q.cap = cap;
        if (noise) q.noise = *noise;
        if (filt) q.filt = *filt;
        return launch(st, dtype, (noise ? 2 : 1) + (filt ? 2 : 0), q);
    }
    int scores(hipStream_t st, int r0, int n, float* C, long ldv) const {
        Itk16Params q = p;
        q.n_rows = n; q.x16 = p.x16 + (long)r0 * p.ldp; q.C = C; q.ldc = ldv;
        return launch(st, dtype, 0, q);
    }
};

}  // namespace

int t4r_itk16_round_rows(hipStream_t st, int dtype, const float* src, long ld, long rows, int D, uint16_t* dst, long ldp) {
    const int chunks = (int)(ldp / 8);
    const int vec = ((uintptr_t)src % 16 == 0 && ld % 4 == 0) ? 1 : 0;
    const long n = rows * chunks;
    const dim3 grid((unsigned)((n + 255) / 256));
    return itk16_dispatch(dtype, [&](auto dt) {
        hipLaunchKernelGGL(itk16_round_rows_kernel<decltype(dt)::value>, grid, dim3(256), 0, st, src, ld, rows, D, dst, ldp, chunks,
                           vec);
        T4R_LAUNCH_CHECK();
        return 0;
    });
}

extern "C" int t4r_item_table_image_ld(int D) { return D > 0 ? (int)itk16_image_ld(D) : 0; }

extern "C" int t4r_item_topk_h16_supported(int D) { return itk16_supported(D) ? 1 : 0; }

extern "C" int t4r_item_table_pack_h16(void* stream, const float* W, long ldw, int V, int D, int dtype, void* image, long ldp) {
    if (V == 0) return 0;
    T4R_CHECK_ARG(V > 0 && D > 0 && W && image && ldw >= D, "item_table_pack_h16: bad arguments");
    ITK16_CHECK_IMAGE("item_table_pack_h16");
    // a wider pitch is zero-filled to its end
    return t4r_itk16_round_rows((hipStream_t)stream, dtype, W, ldw, V, D, (uint16_t*)image, ldp) ? -1 : 0;
}

// workspace: n_rows * t4r_item_table_image_ld(D) * 2 bytes (the 16-bit image of x), 16-byte aligned
extern "C" int t4r_item_scores_h16(void* stream, int n_rows, int V, int D, float alpha, const float* X, long ldx,
                                   const void* image, long ldp, int dtype, float* C, long ldc, void* workspace, long ws_bytes) {
    if (n_rows == 0 || V == 0) return 0;
    T4R_CHECK_ARG(n_rows > 0 && V > 0 && D > 0 && X && image && C, "item_scores_h16: bad arguments");
    T4R_CHECK_ARG(itk16_supported(D), "item_scores_h16: 1 <= D <= 512 (t4r_item_topk_h16_supported)");
    T4R_CHECK_ARG(ldx >= D && ldc >= V, "item_scores_h16: row pitch below the row length");
    ITK16_CHECK_IMAGE("item_scores_h16");
    const long kp = itk16_image_ld(D);
    T4R_CHECK_ARG(workspace && ws_bytes >= (long)n_rows * kp * 2 && (uintptr_t)workspace % 16 == 0,
                  "item_scores_h16: workspace below n_rows * t4r_item_table_image_ld(D) * 2 bytes or not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    uint16_t* x16 = (uint16_t*)workspace;
    int rc = t4r_itk16_round_rows(st, dtype, X, ldx, n_rows, D, x16, kp);
    if (rc) return rc;
    Itk16Params p = {};
    p.n_rows = n_rows; p.n_items = V; p.ldp = (int)kp; p.x16 = x16; p.img = (const uint16_t*)image; p.ldi = ldp; p.stride = 1;
    p.alpha = alpha; p.C = C; p.ldc = ldc;
    return launch(st, dtype, 0, p);
}

extern "C" long t4r_item_topk_h16_ws_bytes(int n_rows, int V, int D, int k) {
    if (n_rows <= 0 || V <= 0 || D <= 0 || k < 1) return 0;
    return (long)make_plan(n_rows, V, k, 0, (size_t)n_rows * itk16_image_ld(D) * 2).total;
}

// host_stats: as t4r_item_topk_f32
extern "C" int t4r_item_topk_h16(void* stream, int n_rows, int V, int D, float alpha, const float* X, long ldx, const void* image,
                                 long ldp, int dtype, int k, float* out_val, long* out_idx, void* workspace, long ws_bytes,
                                 long* host_stats) {
    if (n_rows == 0) return 0;
    T4R_CHECK_ARG(n_rows > 0 && V > 0 && D > 0 && X && image && out_val && out_idx, "item_topk_h16: bad arguments");
    T4R_CHECK_ARG(itk16_supported(D), "item_topk_h16: 1 <= D <= 512 (t4r_item_topk_h16_supported)");
    T4R_CHECK_ARG(k >= 1 && k <= ITK_MAX_K && k <= V, "item_topk_h16: 1 <= k <= min(256, V)");
    T4R_CHECK_ARG(ldx >= D, "item_topk_h16: row pitch below D");
    ITK16_CHECK_IMAGE("item_topk_h16");
    const long kp = itk16_image_ld(D);
    const Plan pl = make_plan(n_rows, V, k, 0, (size_t)n_rows * kp * 2);
    T4R_CHECK_ARG(workspace && ws_bytes >= (long)pl.total && (uintptr_t)workspace % 16 == 0,
                  "item_topk_h16: workspace too small (t4r_item_topk_h16_ws_bytes) or not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    uint16_t* x16 = (uint16_t*)((char*)workspace + pl.off_x);
    int rc = t4r_itk16_round_rows(st, dtype, X, ldx, n_rows, D, x16, kp);
    if (rc) return rc;
    Itk16Head head = {dtype, {}};
    Itk16Params& p = head.p;
    p.n_rows = n_rows; p.n_items = V; p.ldp = (int)kp; p.x16 = x16; p.img = (const uint16_t*)image; p.ldi = ldp; p.stride = 1;
    p.alpha = alpha;
    return itk_run("item_topk_h16", st, pl, workspace, n_rows, V, k, out_val, out_idx, host_stats, head);
}

extern "C" long t4r_item_sample_h16_ws_bytes(int n_rows, int V, int D, int k) { return t4r_item_topk_h16_ws_bytes(n_rows, V, D, k); }

// t4r_item_topk_h16 over fp32(score + g(row0 + row, item)) (include/t4r_hip_sampling.h)
extern "C" int t4r_item_sample_h16(void* stream, int n_rows, int V, int D, float alpha, const float* X, long ldx,
                                   const void* image, long ldp, int dtype, int k, float* out_val, long* out_idx, void* workspace,
                                   long ws_bytes, long* host_stats, long row0, unsigned long long seed,
                                   unsigned long long ctr_hi) {
    if (n_rows == 0) return 0;
    T4R_CHECK_ARG(n_rows > 0 && V > 0 && D > 0 && X && image && out_val && out_idx, "item_sample_h16: bad arguments");
    T4R_CHECK_ARG(itk16_supported(D), "item_sample_h16: 1 <= D <= 512 (t4r_item_topk_h16_supported)");
    T4R_CHECK_ARG(k >= 1 && k <= ITK_MAX_K && k <= V, "item_sample_h16: 1 <= k <= min(256, V)");
    T4R_CHECK_ARG(ldx >= D, "item_sample_h16: row pitch below D");
    T4R_CHECK_ARG(row0 >= 0, "item_sample_h16: row0 must not be negative");
    ITK16_CHECK_IMAGE("item_sample_h16");
    const long kp = itk16_image_ld(D);
    const Plan pl = make_plan(n_rows, V, k, 0, (size_t)n_rows * kp * 2);
    T4R_CHECK_ARG(workspace && ws_bytes >= (long)pl.total && (uintptr_t)workspace % 16 == 0,
                  "item_sample_h16: workspace too small (t4r_item_sample_h16_ws_bytes) or not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    uint16_t* x16 = (uint16_t*)((char*)workspace + pl.off_x);
    int rc = t4r_itk16_round_rows(st, dtype, X, ldx, n_rows, D, x16, kp);
    if (rc) return rc;
    ItkNoisyHead<Itk16Head> head = {{dtype, {}}, {seed, ctr_hi, row0}, n_rows, V};
    Itk16Params& p = head.head.p;
    p.n_rows = n_rows; p.n_items = V; p.ldp = (int)kp; p.x16 = x16; p.img = (const uint16_t*)image; p.ldi = ldp; p.stride = 1;
    p.alpha = alpha;
    return itk_run("item_sample_h16", st, pl, workspace, n_rows, V, k, out_val, out_idx, host_stats, head);
}

// The two heads above under an item filter (include/t4r_hip_filter.h): noise null = t4r_item_topk_filtered_h16
static int itk16_filtered(const char* name, void* stream, int n_rows, int V, int D, float alpha, const float* X, long ldx,
                          const void* image, long ldp, int dtype, int k, float* out_val, long* out_idx, void* workspace,
                          long ws_bytes, long* host_stats, const GumbelCfg* noise, const ItkFilter& filt) {
    auto bad = [&](const char* what) {
        t4r_set_error((std::string(name) + ": " + what).c_str());
        return -1;
    };
    if (n_rows == 0) return 0;
    if (!(n_rows > 0 && V > 0 && D > 0 && X && image && out_val && out_idx)) return bad("bad arguments");
    if (!itk16_supported(D)) return bad("1 <= D <= 512 (t4r_item_topk_h16_supported)");
    if (!(k >= 1 && k <= ITK_MAX_K && k <= V)) return bad("1 <= k <= min(256, V)");
    if (ldx < D) return bad("row pitch below D");
    if (noise && noise->row0 < 0) return bad("row0 must not be negative");
    if (dtype != 2 && dtype != 3) return bad("dtype is 2 (bf16) or 3 (fp16), the codes of T4R_GEMM_PREC");
    if (!(ldp >= itk16_image_ld(D) && ldp % 8 == 0 && (uintptr_t)image % 16 == 0))
        return bad("image rows must be 16-byte aligned with pitch >= t4r_item_table_image_ld(D)");
    if (t4r_item_filter_check(name, filt.allow_bits, filt.excl, filt.n_excl, filt.ld_excl)) return -1;
    const long kp = itk16_image_ld(D);
    const Plan pl = make_plan(n_rows, V, k, 0, (size_t)n_rows * kp * 2);
    if (!(workspace && ws_bytes >= (long)pl.total && (uintptr_t)workspace % 16 == 0))
        return bad("workspace too small (the unfiltered entry's ws_bytes) or not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    uint16_t* x16 = (uint16_t*)((char*)workspace + pl.off_x);
    const int rc = t4r_itk16_round_rows(st, dtype, X, ldx, n_rows, D, x16, kp);
    if (rc) return rc;
    Itk16Head base = {dtype, {}};
    Itk16Params& p = base.p;
    p.n_rows = n_rows; p.n_items = V; p.ldp = (int)kp; p.x16 = x16; p.img = (const uint16_t*)image; p.ldi = ldp; p.stride = 1;
    p.alpha = alpha;
    if (!noise) return itk_run_filtered(name, st, pl, workspace, n_rows, V, k, out_val, out_idx, host_stats, base, filt);
    const ItkNoisyHead<Itk16Head> noisy = {base, *noise, n_rows, V};
    return itk_run_filtered(name, st, pl, workspace, n_rows, V, k, out_val, out_idx, host_stats, noisy, filt);
}

extern "C" int t4r_item_topk_filtered_h16(void* stream, int n_rows, int V, int D, float alpha, const float* X, long ldx,
                                          const void* image, long ldp, int dtype, int k, float* out_val, long* out_idx,
                                          void* workspace, long ws_bytes, long* host_stats, const unsigned* allow_bits,
                                          const long* excl, int n_excl, long ld_excl) {
    return itk16_filtered("item_topk_filtered_h16", stream, n_rows, V, D, alpha, X, ldx, image, ldp, dtype, k, out_val, out_idx,
                          workspace, ws_bytes, host_stats, nullptr, ItkFilter{allow_bits, excl, n_excl, ld_excl});
}

extern "C" int t4r_item_sample_filtered_h16(void* stream, int n_rows, int V, int D, float alpha, const float* X, long ldx,
                                            const void* image, long ldp, int dtype, int k, float* out_val, long* out_idx,
                                            void* workspace, long ws_bytes, long* host_stats, long row0,
                                            unsigned long long seed, unsigned long long ctr_hi, const unsigned* allow_bits,
                                            const long* excl, int n_excl, long ld_excl) {
    const GumbelCfg noise = {seed, ctr_hi, row0};
    return itk16_filtered("item_sample_filtered_h16", stream, n_rows, V, D, alpha, X, ldx, image, ldp, dtype, k, out_val, out_idx,
                          workspace, ws_bytes, host_stats, &noise, ItkFilter{allow_bits, excl, n_excl, ld_excl});
}
