// Fused top-k inference head: (values [N, k], ids [N, k]) of the k best items of alpha * X[N, D] @ W[V, D]^T per row, without
// an [N, V] score matrix.  Replaces the last-item scores + torch.topk of a served model
// (transformers4rec/torch/model/prediction_task.py:452-470, :664) where the scores are too large to exist.
//
// The result is the one "scores by the fp32-core GEMM, then t4r_topk" gives, bit for bit: both products below run form 0
// (fp32 operands on the fp32 matrix cores), an output element's bits do not depend on its tile position or tile size, and the
// order is t4r_topk's (value descending, ties to the lower index).
//
//   1. threshold  a STRIDED sample of M item rows (v = 0, s, 2 s, ...: ids are often sorted by popularity, a prefix would sit
//                 far above the rest) is gathered and scored with the ordinary GEMM into S [N, M]; t4r_topk takes each row's k
//                 best sampled scores.  The k-th of them, t0[row], is a lower bound of the row's true k-th largest score: k real
//                 scores with exactly these bits exist.
//   2. collect    one pass over the table: the GEMM kernel with the collect epilogue (gemm_kernel.h, FEAT bit 3) appends
//                 (score, item) of every score >= t0[row] to the row's candidate list, one slot-counter atomic per 32-lane
//                 half that found something.  About k V / M candidates per row.
//   3. select     one workgroup per row runs t4r_topk's own three steps on the list (slice maxima -> tighter bound t1 -> the
//                 few candidates >= t1 in LDS -> rank by (value desc, item asc)).  Arrival order in the list only moves t1
//                 between two valid bounds; the k winners and their order do not depend on it.
//   4. overflow   a row that had more candidates than its list holds (constant tables, thousands of duplicates of the best
//                 item), fewer than k (a NaN score), or more than the LDS list after t1 is flagged.  The flag count is read back
//                 once per call (inference: one 4-byte device-to-host read) and flagged rows are recomputed through the
//                 materialised path -- scores of those rows into the (now free) candidate region, then t4r_topk -- so the result
//                 is exact for every input.
//
// The four steps and the overflow bookkeeping are itk_run (item_topk_plan.h), shared with item_topk_h16.hip; this file holds the
// fp32 head's three products (Itk32Head), the gather of the sample and the select kernel.
// The SAMPLING form of the same call (t4r_item_sample_f32, include/t4r_hip_sampling.h) is the same four steps over the
// perturbed score fp32(s + g(row, item)) (gumbel_noise.h): ItkNoisyHead (item_topk_plan.h) around this head.
#include "item_topk_plan.h"
#include "t4r_internal.h"

namespace {

__global__ __launch_bounds__(256) void itk_sample_rows_kernel(const float* __restrict__ W, long ldw, int stride,
                                                               float* __restrict__ out, int M, int D) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)M * D) return;
    const long r = i / D, c = i % D;
    out[i] = W[r * stride * ldw + c];
}

// step 3 (and the flagging of step 4) for one row per workgroup
__global__ __launch_bounds__(256) void itk_select_kernel(const float* __restrict__ cand_val, const int* __restrict__ cand_idx,
                                                          const int* __restrict__ count, int cap, int k,
                                                          float* __restrict__ out_val, long* __restrict__ out_idx,
                                                          int* __restrict__ n_flagged, int* __restrict__ flagged) {
    __shared__ float lv[ITK_LDS_CAP];
    __shared__ int li[ITK_LDS_CAP];
    __shared__ float tmax[256];
    __shared__ float t1s;
    __shared__ int cnt;
    const int row = blockIdx.x, tid = threadIdx.x;
    const int C = count[row];
    const float* cv = cand_val + (long)row * cap;
    const int* ci = cand_idx + (long)row * cap;
    auto flag_row = [&]() {
        if (tid == 0) flagged[atomicAdd(n_flagged, 1)] = row;
    };
    if (C > cap || C < k) { flag_row(); return; }            // workgroup-uniform
    float m = -INFINITY;
    for (int c = tid; c < C; c += 256) m = fmaxf(m, cv[c]);
    tmax[tid] = m;
    if (tid == 0) cnt = 0;
    __syncthreads();
    {
        // C >= k candidates dealt round-robin: at least k slices are non-empty, so the k-th largest slice maximum is a real score
        int rank = 0;
        for (int o = 0; o < 256; ++o) {
            const float v = tmax[o];
            rank += (v > m || (v == m && o < tid)) ? 1 : 0;
        }
        if (rank == k - 1) t1s = m;
    }
    __syncthreads();
    const float t1 = t1s;
    for (int c = tid; c < C; c += 256) {
        const float v = cv[c];
        if (v >= t1) {
            const int slot = atomicAdd(&cnt, 1);
            if (slot < ITK_LDS_CAP) { lv[slot] = v; li[slot] = ci[c]; }
        }
    }
    __syncthreads();
    const int L = cnt;
    if (L > ITK_LDS_CAP) { flag_row(); return; }             // workgroup-uniform
    for (int c = tid; c < L; c += 256) {
        const float v = lv[c];
        const int i = li[c];
        int rank = 0;
        for (int o = 0; o < L; ++o) {
            const float v2 = lv[o];
            rank += (v2 > v || (v2 == v && li[o] < i)) ? 1 : 0;
        }
        if (rank < k) {
            out_val[(long)row * k + rank] = v;
            out_idx[(long)row * k + rank] = i;
        }
    }
}

// the fp32 table on the fp32 matrix cores (form 0): the head object of itk_run
struct Itk32Head {
    int n_rows, V, D;
    float alpha;
    const float* X; long ldx;
    const float* W; long ldw;
    float* wsamp;                   // [pl.M, D]: the gathered sample rows

    int sample(hipStream_t st, const Plan& pl, float* S) const {
        const long md = (long)pl.M * D;
        hipLaunchKernelGGL(itk_sample_rows_kernel, dim3((unsigned)((md + 255) / 256)), dim3(256), 0, st, W, ldw, pl.stride, wsamp,
                           pl.M, D);
        T4R_LAUNCH_CHECK();
        return t4r_gemm_fp32_nt_launch(st, n_rows, pl.M, D, alpha, X, ldx, wsamp, D, S, pl.ldS);
    }
    int collect(hipStream_t st, const float* thr, long thr_ld, int* count, float* cand_val, int* cand_idx, int cap,
                const GumbelCfg* noise = nullptr, const ItkFilter* filt = nullptr) const {
        if (filt)
            return t4r_gemm_topk_collect_filtered_launch(st, n_rows, V, D, alpha, X, ldx, W, ldw, thr, thr_ld, count, cand_val,
                                                         cand_idx, cap, noise, filt);
        return t4r_gemm_topk_collect_launch(st, n_rows, V, D, alpha, X, ldx, W, ldw, thr, thr_ld, count, cand_val, cand_idx, cap,
                                            noise);
    }
    int scores(hipStream_t st, int r0, int n, float* C, long ldv) const {
        return t4r_gemm_fp32_nt_launch(st, n, V, D, alpha, X + (long)r0 * ldx, ldx, W, ldw, C, ldv);
    }
};

}  // namespace

// step 3 for itk_run (item_topk_plan.h): one select kernel, one set of flags for both heads
int t4r_itk_select_launch(hipStream_t st, int n_rows, const float* cand_val, const int* cand_idx, const int* count, int cap, int k,
                          float* out_val, long* out_idx, int* n_flagged, int* flagged) {
    hipLaunchKernelGGL(itk_select_kernel, dim3(n_rows), dim3(256), 0, st, cand_val, cand_idx, count, cap, k, out_val, out_idx,
                       n_flagged, flagged);
    T4R_LAUNCH_CHECK();
    return 0;
}

extern "C" long t4r_item_topk_ws_bytes(int n_rows, int V, int D, int k) {
    if (n_rows <= 0 || V <= 0 || D <= 0 || k < 1) return 0;
    return (long)make_plan(n_rows, V, k, (size_t)D * 4, 0).total;
}

// host_stats (host memory, 8 longs, may be null): what this call did -- [0] rows that took the materialised overflow path,
// [1] sampled item rows M, [2] list capacity per row; and, only if host_stats[7] != 0 on entry (tools: it costs an [n_rows]
// device-to-host copy), [3] / [4] = sum / maximum over rows of the candidate counts.  The library keeps no record of its own.
extern "C" int t4r_item_topk_f32(void* stream, int n_rows, int V, int D, float alpha, const float* X, long ldx,
                                 const float* W, long ldw, int k, float* out_val, long* out_idx, void* workspace,
                                 long ws_bytes, long* host_stats) {
    if (n_rows == 0) return 0;
    T4R_CHECK_ARG(n_rows > 0 && V > 0 && D > 0 && X && W && out_val && out_idx, "item_topk: bad arguments");
    T4R_CHECK_ARG(k >= 1 && k <= ITK_MAX_K && k <= V, "item_topk: 1 <= k <= min(256, V)");
    T4R_CHECK_ARG(ldx >= D && ldw >= D, "item_topk: row pitch below D");
    const Plan pl = make_plan(n_rows, V, k, (size_t)D * 4, 0);
    T4R_CHECK_ARG(workspace && ws_bytes >= (long)pl.total && (uintptr_t)workspace % 16 == 0,
                  "item_topk: workspace too small (t4r_item_topk_ws_bytes) or not 16-byte aligned");
    Itk32Head head = {n_rows, V, D, alpha, X, ldx, W, ldw, (float*)((char*)workspace + pl.off_wsamp)};
    return itk_run("item_topk", (hipStream_t)stream, pl, workspace, n_rows, V, k, out_val, out_idx, host_stats, head);
}

extern "C" long t4r_item_sample_ws_bytes(int n_rows, int V, int D, int k) { return t4r_item_topk_ws_bytes(n_rows, V, D, k); }

// t4r_item_topk_f32 over fp32(score + g(row0 + row, item)): Gumbel top-k, a sample of k items without replacement in proportion
// to softmax(scores) (include/t4r_hip_sampling.h)
extern "C" int t4r_item_sample_f32(void* stream, int n_rows, int V, int D, float alpha, const float* X, long ldx,
                                   const float* W, long ldw, int k, float* out_val, long* out_idx, void* workspace,
                                   long ws_bytes, long* host_stats, long row0, unsigned long long seed,
                                   unsigned long long ctr_hi) {
    if (n_rows == 0) return 0;
    T4R_CHECK_ARG(n_rows > 0 && V > 0 && D > 0 && X && W && out_val && out_idx, "item_sample: bad arguments");
    T4R_CHECK_ARG(k >= 1 && k <= ITK_MAX_K && k <= V, "item_sample: 1 <= k <= min(256, V)");
    T4R_CHECK_ARG(ldx >= D && ldw >= D, "item_sample: row pitch below D");
    T4R_CHECK_ARG(row0 >= 0, "item_sample: row0 must not be negative");
    const Plan pl = make_plan(n_rows, V, k, (size_t)D * 4, 0);
    T4R_CHECK_ARG(workspace && ws_bytes >= (long)pl.total && (uintptr_t)workspace % 16 == 0,
                  "item_sample: workspace too small (t4r_item_sample_ws_bytes) or not 16-byte aligned");
    const Itk32Head base = {n_rows, V, D, alpha, X, ldx, W, ldw, (float*)((char*)workspace + pl.off_wsamp)};
    ItkNoisyHead<Itk32Head> head = {base, {seed, ctr_hi, row0}, n_rows, V};
    return itk_run("item_sample", (hipStream_t)stream, pl, workspace, n_rows, V, k, out_val, out_idx, host_stats, head);
}

// The two entries above under an item filter (include/t4r_hip_filter.h): noise null = t4r_item_topk_filtered_f32
static int itk32_filtered(const char* name, void* stream, int n_rows, int V, int D, float alpha, const float* X, long ldx,
                          const float* W, long ldw, int k, float* out_val, long* out_idx, void* workspace, long ws_bytes,
                          long* host_stats, const GumbelCfg* noise, const ItkFilter& filt) {
    auto bad = [&](const char* what) {
        t4r_set_error((std::string(name) + ": " + what).c_str());
        return -1;
    };
    if (n_rows == 0) return 0;
    if (!(n_rows > 0 && V > 0 && D > 0 && X && W && out_val && out_idx)) return bad("bad arguments");
    if (!(k >= 1 && k <= ITK_MAX_K && k <= V)) return bad("1 <= k <= min(256, V)");
    if (!(ldx >= D && ldw >= D)) return bad("row pitch below D");
    if (noise && noise->row0 < 0) return bad("row0 must not be negative");
    if (t4r_item_filter_check(name, filt.allow_bits, filt.excl, filt.n_excl, filt.ld_excl)) return -1;
    const Plan pl = make_plan(n_rows, V, k, (size_t)D * 4, 0);
    if (!(workspace && ws_bytes >= (long)pl.total && (uintptr_t)workspace % 16 == 0))
        return bad("workspace too small (the unfiltered entry's ws_bytes) or not 16-byte aligned");
    const Itk32Head base = {n_rows, V, D, alpha, X, ldx, W, ldw, (float*)((char*)workspace + pl.off_wsamp)};
    if (!noise) return itk_run_filtered(name, (hipStream_t)stream, pl, workspace, n_rows, V, k, out_val, out_idx, host_stats, base, filt);
    const ItkNoisyHead<Itk32Head> noisy = {base, *noise, n_rows, V};
    return itk_run_filtered(name, (hipStream_t)stream, pl, workspace, n_rows, V, k, out_val, out_idx, host_stats, noisy, filt);
}

extern "C" int t4r_item_topk_filtered_f32(void* stream, int n_rows, int V, int D, float alpha, const float* X, long ldx,
                                          const float* W, long ldw, int k, float* out_val, long* out_idx, void* workspace,
                                          long ws_bytes, long* host_stats, const unsigned* allow_bits, const long* excl,
                                          int n_excl, long ld_excl) {
    return itk32_filtered("item_topk_filtered", stream, n_rows, V, D, alpha, X, ldx, W, ldw, k, out_val, out_idx, workspace,
                          ws_bytes, host_stats, nullptr, ItkFilter{allow_bits, excl, n_excl, ld_excl});
}

extern "C" int t4r_item_sample_filtered_f32(void* stream, int n_rows, int V, int D, float alpha, const float* X, long ldx,
                                            const float* W, long ldw, int k, float* out_val, long* out_idx, void* workspace,
                                            long ws_bytes, long* host_stats, long row0, unsigned long long seed,
                                            unsigned long long ctr_hi, const unsigned* allow_bits, const long* excl, int n_excl,
                                            long ld_excl) {
    const GumbelCfg noise = {seed, ctr_hi, row0};
    return itk32_filtered("item_sample_filtered", stream, n_rows, V, D, alpha, X, ldx, W, ldw, k, out_val, out_idx, workspace,
                          ws_bytes, host_stats, &noise, ItkFilter{allow_bits, excl, n_excl, ld_excl});
}
