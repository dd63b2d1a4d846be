// Row-sparse ("lazy") Adam for embedding tables (C ABI: include/t4r_hip_rowadam.h).
//
// Replaces the torch.optim.Adam.step of Model.fit (transformers4rec/torch/model/base.py:669-718), restricted to the table
// rows that have a gradient in this step -- what torch.optim.SparseAdam does for an nn.Embedding(sparse=True).
//
// The dense route (optim.hip / elementwise.hip over a flat bucket) keeps a zeroed [V, D] gradient, scatters the (ids, rows)
// the backward produced into it and streams param, grad and both moments of EVERY row: 7 V D 4 bytes whatever the batch
// touched.  Here the gradient never becomes dense.  From the sorted lookups (t4r_sort_ids: keys ascending, stable, invalid
// lookups carry the key V and come last):
//   1. row_heads_kernel marks the first position of every run of a valid key; an inclusive scan of the marks [hipCUB] numbers
//      the distinct rows 0 .. U-1 in key order; row_ranks_kernel writes, per sorted position, the rank of its key (invalid:
//      n, the "skip" key of stage 2) and, per rank, the table row.  U stays on the device (the last element of the scan).
//   2. the segmented sum of seg_sum_kernel.h -- the device code and the geometry of t4r_embedding_bwd_sorted, so the same
//      summation order and the same bits -- with the ranks as keys, ASSIGNING into a compact [U, D] buffer.  A run of any
//      length is cut at super-chunk borders and its partials are combined by pass B: one popular item does not serialise
//      the launch on one wave.
//   3. row_adam_kernel: one thread per 16 bytes (or per float) of the U rows; gathers the row's param and moments, runs
//      adamw_element (adam_kernel.h, coefficient 1) and writes the three back.  Grid sized from n; threads past U rows exit.
// No float atomics, no host read, nothing allocated: all scratch is carved from the caller's workspace.
//
// The same three stages cut after the second (C ABI: include/t4r_hip_rowclip.h), for global-norm clipping over dense buckets
// and lazily stepped tables together: t4r_row_adam_reduce runs 1 and 2 and then row_sumsq_kernel, the sum of squares in double
// of the U D floats of the compact buffer -- the non-zero rows of the dense gradient clip_grad_norm_ would have seen -- as
// per-workgroup partials that join the buckets' (optim.hip); t4r_row_adam_apply runs 3 with the coefficient t4r_grad_clip_coef
// left on the device.  The workspace carries heads, ranks and the compact rows from one call to the other: one more read of
// 4 U D bytes and one more launch than the unclipped step.
// Algorithmic bytes: n (4 key + 4 perm) + ~16 n of stage 1 + n D 4 gradient rows + 2 U D 4 compact buffer + 6 U D 4 table rows.
#include "t4r_common.h"
#include "adam_kernel.h"
#include "seg_sum_kernel.h"
#include "sumsq_kernel.h"
#include <hipcub/hipcub.hpp>
#include <math.h>

static size_t ra_al256(size_t b) { return (b + 255) & ~(size_t)255; }

__global__ __launch_bounds__(256) void row_heads_kernel(const int* __restrict__ keys, long n, int V, int* __restrict__ heads) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int k = keys[i];
    heads[i] = (k >= 0 && k < V && (i == 0 || keys[i - 1] != k)) ? 1 : 0;
}

// incl = inclusive scan of heads: a valid position's rank is incl - 1; the run's first position also records the table row
__global__ __launch_bounds__(256) void row_ranks_kernel(const int* __restrict__ keys, const int* __restrict__ heads,
                                                         const int* __restrict__ incl, long n, int V, int* __restrict__ rank,
                                                         int* __restrict__ urow) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int k = keys[i];
    if (k < 0 || k >= V) { rank[i] = (int)n; return; }
    const int r = incl[i] - 1;
    rank[i] = r;
    if (heads[i]) urow[r] = k;
}

// Gather / scatter of whole rows: a row's D floats are contiguous in param, exp_avg, exp_avg_sq and in the compact gradient,
// so the D / VEC threads of a row read and write full 16-byte (VEC = 4) segments side by side; rows themselves are anywhere in
// the table, which makes the pass latency bound -- four independent loads per thread are issued before the first is used and
// the kernel holds few registers, so that many waves per SIMD keep loads in flight.
// CLIP (t4r_row_adam_apply): the coefficient of the global norm, read from device memory once per thread (null: 1), multiplies
// the gradient after grad_scale -- adamw_element's two roundings.  Without it the instructions are the unclipped step's.
template <int VEC, bool CLIP>
__global__ __launch_bounds__(256) void row_adam_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                        const float* __restrict__ g, const int* __restrict__ urow,
                                                        const int* __restrict__ n_rows, int D, float lr, float b1, float b2,
                                                        float eps, float wd, float bc1, float bc2_sqrt, float grad_scale,
                                                        int decoupled, float decay_factor, const float* __restrict__ clip_coef) {
    const int per_row = D / VEC;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long u = e / per_row;
    if (u >= (long)*n_rows) return;
    const int c = (int)(e - u * per_row) * VEC;
    const long at = (long)urow[u] * D + c;
    const float step_size = lr / bc1;
    const float coef = CLIP && clip_coef ? *clip_coef : 1.f;
    if (VEC == 4) {
        float4 gg = *reinterpret_cast<const float4*>(g + u * D + c);
        float4 pp = *reinterpret_cast<float4*>(p + at);
        float4 mm = *reinterpret_cast<float4*>(m + at);
        float4 vv = *reinterpret_cast<float4*>(v + at);
        float* P = &pp.x; float* G = &gg.x; float* M = &mm.x; float* Vv = &vv.x;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            adamw_element(P[i], G[i], M[i], Vv[i], step_size, b1, b2, eps, wd, bc2_sqrt, grad_scale, coef, decoupled, decay_factor);
        *reinterpret_cast<float4*>(p + at) = pp;
        *reinterpret_cast<float4*>(m + at) = mm;
        *reinterpret_cast<float4*>(v + at) = vv;
    } else {
        float pp = p[at], mm = m[at], vv = v[at];
        adamw_element(pp, g[u * D + c], mm, vv, step_size, b1, b2, eps, wd, bc2_sqrt, grad_scale, coef, decoupled, decay_factor);
        p[at] = pp;
        m[at] = mm;
        v[at] = vv;
    }
}

struct RowAdamLayout { size_t heads, incl, rank, urow, tmp, tmp_bytes, compact, partial, total; };
static RowAdamLayout row_adam_layout(long n, int D) {
    RowAdamLayout l;
    size_t o = 0;
    auto take = [&](size_t b) { size_t at = o; o += ra_al256(b); return at; };
    l.heads = take((size_t)n * 4);
    l.incl = take((size_t)n * 4);
    l.rank = take((size_t)n * 4);
    l.urow = take((size_t)n * 4);
    size_t sb = 0;
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, sb, (int*)nullptr, (int*)nullptr, (int)n);
    l.tmp_bytes = sb;
    l.tmp = take(sb);
    l.compact = take((size_t)n * D * 4);        // U <= n distinct rows; U is known on the device only
    // two partial rows per super-chunk at the SHORTEST super-chunk (seg_S = 1): an upper bound of seg_ws_floats that grows with n
    const size_t CH = (size_t)seg_CH(D);
    l.partial = take((((size_t)n + CH - 1) / CH) * 2 * (size_t)D * 4);
    l.total = o;
    return l;
}

extern "C" long t4r_row_adam_ws_bytes(long n, int D) {
    if (n <= 0 || D < 1 || n >= (1L << 31) - 1) return 0;
    return (long)row_adam_layout(n, D).total;
}

// stages 1 and 2: heads, scan, ranks, then the segmented sum into the compact buffer.  0, or -1 with the error set.
static int row_adam_sum_rows(hipStream_t st, const RowAdamLayout& l, char* w, long V, int D, const int* keys, const int* perm,
                             const float* grad_rows, long ld_grad, long n) {
    int* heads = (int*)(w + l.heads);
    int* incl = (int*)(w + l.incl);
    int* rank = (int*)(w + l.rank);
    int* urow = (int*)(w + l.urow);
    float* compact = (float*)(w + l.compact);
    float* partial = (float*)(w + l.partial);
    const unsigned gn = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(row_heads_kernel, dim3(gn), dim3(256), 0, st, keys, n, (int)V, heads);
    size_t tb = l.tmp_bytes;
    if (hipcub::DeviceScan::InclusiveSum(w + l.tmp, tb, heads, incl, (int)n, st) != hipSuccess) {
        t4r_set_error("row_adam: device scan failed");
        return -1;
    }
    hipLaunchKernelGGL(row_ranks_kernel, dim3(gn), dim3(256), 0, st, keys, heads, incl, n, (int)V, rank, urow);
    // the ranks are the keys: distinct rows 0 .. U-1 of the compact buffer, n = "no gradient"
    seg_sum_launch<true>(st, grad_rows, rank, perm, compact, partial, n, (int)ld_grad, 0, D, (int)n, 1);
    return 0;
}

static int row_adam_vec(int D, const float* param, const float* exp_avg, const float* exp_avg_sq) {
    return (D % 4 == 0 && ((uintptr_t)param | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16 == 0) ? 4 : 1;
}

// stage 3 over the compact buffer of `w`; CLIP: with the device coefficient (t4r_row_adam_apply)
template <bool CLIP>
static void row_adam_update(hipStream_t st, const RowAdamLayout& l, char* w, float* param, float* exp_avg, float* exp_avg_sq, int D,
                            long n, int VEC, long adam_blocks, int step, float lr, float beta1, float beta2, float eps,
                            float weight_decay, int decoupled, float grad_scale, const float* clip_coef) {
    const int* incl = (const int*)(w + l.incl);
    const int* urow = (const int*)(w + l.urow);
    const float* compact = (const float*)(w + l.compact);
    // as t4r_adamw_step: the bias corrections, and the decay factor with them, in double from the float arguments, rounded once
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    const float bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    const float factor = (float)(1.0 - (double)lr * (double)weight_decay);
    if (VEC == 4)
        hipLaunchKernelGGL((row_adam_kernel<4, CLIP>), dim3((unsigned)adam_blocks), dim3(256), 0, st, param, exp_avg, exp_avg_sq, compact,
                           urow, incl + (n - 1), D, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale, decoupled, factor,
                           clip_coef);
    else
        hipLaunchKernelGGL((row_adam_kernel<1, CLIP>), dim3((unsigned)adam_blocks), dim3(256), 0, st, param, exp_avg, exp_avg_sq, compact,
                           urow, incl + (n - 1), D, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale, decoupled, factor,
                           clip_coef);
}

extern "C" int t4r_row_adam_step(void* stream, float* param, float* exp_avg, float* exp_avg_sq, long V, int D, const int* keys,
                                 const int* perm, const float* grad_rows, long ld_grad, long n, int step, float lr, float beta1,
                                 float beta2, float eps, float weight_decay, int decoupled, float grad_scale, void* ws,
                                 long ws_bytes) {
    T4R_CHECK_ARG(n >= 0, "row_adam: n must not be negative");
    T4R_CHECK_ARG(D >= 1, "row_adam: D must be at least 1");
    T4R_CHECK_ARG(V >= 1 && V < (1L << 31) - 1, "row_adam: V must be at least 1 and fit 31 bits");
    T4R_CHECK_ARG(step >= 1, "row_adam: step is 1-based");
    if (n == 0) return 0;
    T4R_CHECK_ARG(param && exp_avg && exp_avg_sq && keys && perm && grad_rows && ws, "row_adam: null pointer");
    T4R_CHECK_ARG(n < (1L << 31) - 1, "row_adam: n must fit 31 bits");
    T4R_CHECK_ARG(ld_grad >= D && ld_grad < (1L << 31), "row_adam: ld_grad must be at least D and fit 31 bits");
    T4R_CHECK_ARG(((uintptr_t)param | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)grad_rows) % 4 == 0,
                  "row_adam: buffers must be 4-byte aligned");
    T4R_CHECK_ARG((uintptr_t)ws % 16 == 0, "row_adam: the workspace must be 16-byte aligned");
    const RowAdamLayout l = row_adam_layout(n, D);
    T4R_CHECK_ARG(ws_bytes >= (long)l.total, "row_adam: workspace too small (t4r_row_adam_ws_bytes)");
    const int VEC = row_adam_vec(D, param, exp_avg, exp_avg_sq);
    const long adam_blocks = (n * (long)(D / VEC) + 255) / 256;
    T4R_CHECK_ARG(adam_blocks < (1L << 31), "row_adam: n * D is too large for one launch");

    hipStream_t st = (hipStream_t)stream;
    if (row_adam_sum_rows(st, l, (char*)ws, V, D, keys, perm, grad_rows, ld_grad, n) != 0) return -1;
    row_adam_update<false>(st, l, (char*)ws, param, exp_avg, exp_avg_sq, D, n, VEC, adam_blocks, step, lr, beta1, beta2, eps,
                           weight_decay, decoupled, grad_scale, nullptr);
    T4R_LAUNCH_CHECK();
    return 0;
}

// ---- include/t4r_hip_rowclip.h: the same step in two halves, with the compact rows' sum of squares in between

// sumsq_block (sumsq_kernel.h: grad_sumsq_kernel's body and order) over the first U D floats of the compact buffer.  The grid
// comes from (n, D) -- the host does not know U --, so a workgroup whose elements all lie past U D adds nothing and stores 0.0:
// every one of the gridDim.x slots is written.
__global__ __launch_bounds__(256) void row_sumsq_kernel(const float* __restrict__ g, const int* __restrict__ n_rows, int D,
                                                         double* __restrict__ part) {
    const double acc = sumsq_block(g, (long)*n_rows * D, sumsq_first(), sumsq_stride());
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

extern "C" long t4r_row_grad_sumsq_parts(long n, int D) {
    if (n <= 0 || D < 1) return 0;
    return sumsq_parts(n * (long)D);
}

extern "C" int t4r_row_adam_reduce(void* stream, long V, int D, const int* keys, const int* perm, const float* grad_rows,
                                   long ld_grad, long n, void* ws, long ws_bytes, double* part) {
    T4R_CHECK_ARG(n >= 0, "row_adam_reduce: n must not be negative");
    T4R_CHECK_ARG(D >= 1, "row_adam_reduce: D must be at least 1");
    T4R_CHECK_ARG(V >= 1 && V < (1L << 31) - 1, "row_adam_reduce: V must be at least 1 and fit 31 bits");
    if (n == 0) return 0;
    T4R_CHECK_ARG(keys && perm && grad_rows && ws && part, "row_adam_reduce: null pointer");
    T4R_CHECK_ARG(n < (1L << 31) - 1, "row_adam_reduce: n must fit 31 bits");
    T4R_CHECK_ARG(ld_grad >= D && ld_grad < (1L << 31), "row_adam_reduce: ld_grad must be at least D and fit 31 bits");
    T4R_CHECK_ARG((uintptr_t)grad_rows % 4 == 0, "row_adam_reduce: grad_rows must be 4-byte aligned");
    T4R_CHECK_ARG((uintptr_t)ws % 16 == 0, "row_adam_reduce: the workspace must be 16-byte aligned");
    T4R_CHECK_ARG((uintptr_t)part % 8 == 0, "row_adam_reduce: part must be 8-byte aligned");
    const RowAdamLayout l = row_adam_layout(n, D);
    T4R_CHECK_ARG(ws_bytes >= (long)l.total, "row_adam_reduce: workspace too small (t4r_row_adam_ws_bytes)");
    T4R_CHECK_ARG((n * (long)D + 255) / 256 < (1L << 31), "row_adam_reduce: n * D is too large for one launch");

    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    if (row_adam_sum_rows(st, l, w, V, D, keys, perm, grad_rows, ld_grad, n) != 0) return -1;
    const long blocks = sumsq_parts(n * (long)D);
    hipLaunchKernelGGL(row_sumsq_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)(w + l.compact),
                       (const int*)(w + l.incl) + (n - 1), D, part);
    if (hipGetLastError() != hipSuccess) { t4r_set_error("row_adam_reduce: launch failed"); return -2; }
    return (int)blocks;
}

extern "C" int t4r_row_adam_apply(void* stream, float* param, float* exp_avg, float* exp_avg_sq, long V, int D, long n, int step,
                                  float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled,
                                  float grad_scale, const float* clip_coef, void* ws, long ws_bytes) {
    T4R_CHECK_ARG(n >= 0, "row_adam_apply: n must not be negative");
    T4R_CHECK_ARG(D >= 1, "row_adam_apply: D must be at least 1");
    T4R_CHECK_ARG(V >= 1 && V < (1L << 31) - 1, "row_adam_apply: V must be at least 1 and fit 31 bits");
    T4R_CHECK_ARG(step >= 1, "row_adam_apply: step is 1-based");
    if (n == 0) return 0;
    T4R_CHECK_ARG(param && exp_avg && exp_avg_sq && ws, "row_adam_apply: null pointer");
    T4R_CHECK_ARG(n < (1L << 31) - 1, "row_adam_apply: n must fit 31 bits");
    T4R_CHECK_ARG(((uintptr_t)param | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 4 == 0,
                  "row_adam_apply: buffers must be 4-byte aligned");
    T4R_CHECK_ARG((uintptr_t)clip_coef % 4 == 0, "row_adam_apply: clip_coef must be 4-byte aligned");
    T4R_CHECK_ARG((uintptr_t)ws % 16 == 0, "row_adam_apply: the workspace must be 16-byte aligned");
    const RowAdamLayout l = row_adam_layout(n, D);
    T4R_CHECK_ARG(ws_bytes >= (long)l.total, "row_adam_apply: workspace too small (t4r_row_adam_ws_bytes)");
    const int VEC = row_adam_vec(D, param, exp_avg, exp_avg_sq);
    const long adam_blocks = (n * (long)(D / VEC) + 255) / 256;
    T4R_CHECK_ARG(adam_blocks < (1L << 31), "row_adam_apply: n * D is too large for one launch");

    row_adam_update<true>((hipStream_t)stream, l, (char*)ws, param, exp_avg, exp_avg_sq, D, n, VEC, adam_blocks, step, lr, beta1,
                          beta2, eps, weight_decay, decoupled, grad_scale, clip_coef);
    T4R_LAUNCH_CHECK();
    return 0;
}
