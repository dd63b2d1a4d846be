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
// Algorithmic bytes: n (4 key + 4 perm) + ~16 n of stage 1 + n D 4 gradient rows + 2 U D 4 compact buffer + 6 U D 4 table rows.
#include "t4r_common.h"
#include "adam_kernel.h"
#include "seg_sum_kernel.h"
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
template <int VEC>
__global__ __launch_bounds__(256) void row_adam_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                        const float* __restrict__ g, const int* __restrict__ urow,
                                                        const int* __restrict__ n_rows, int D, float lr, float b1, float b2,
                                                        float eps, float wd, float bc1, float bc2_sqrt, float grad_scale,
                                                        int decoupled, float decay_factor) {
    const int per_row = D / VEC;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long u = e / per_row;
    if (u >= (long)*n_rows) return;
    const int c = (int)(e - u * per_row) * VEC;
    const long at = (long)urow[u] * D + c;
    const float step_size = lr / bc1;
    if (VEC == 4) {
        float4 gg = *reinterpret_cast<const float4*>(g + u * D + c);
        float4 pp = *reinterpret_cast<float4*>(p + at);
        float4 mm = *reinterpret_cast<float4*>(m + at);
        float4 vv = *reinterpret_cast<float4*>(v + at);
        float* P = &pp.x; float* G = &gg.x; float* M = &mm.x; float* Vv = &vv.x;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            adamw_element(P[i], G[i], M[i], Vv[i], step_size, b1, b2, eps, wd, bc2_sqrt, grad_scale, 1.f, decoupled, decay_factor);
        *reinterpret_cast<float4*>(p + at) = pp;
        *reinterpret_cast<float4*>(m + at) = mm;
        *reinterpret_cast<float4*>(v + at) = vv;
    } else {
        float pp = p[at], mm = m[at], vv = v[at];
        adamw_element(pp, g[u * D + c], mm, vv, step_size, b1, b2, eps, wd, bc2_sqrt, grad_scale, 1.f, decoupled, decay_factor);
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
    const int VEC = (D % 4 == 0 && ((uintptr_t)param | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16 == 0) ? 4 : 1;
    const long adam_blocks = (n * (long)(D / VEC) + 255) / 256;
    T4R_CHECK_ARG(adam_blocks < (1L << 31), "row_adam: n * D is too large for one launch");

    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
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
    // as t4r_adamw_step: the bias corrections, and the decay factor with them, in double from the float arguments, rounded once
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    const float bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    const float factor = (float)(1.0 - (double)lr * (double)weight_decay);
    if (VEC == 4)
        hipLaunchKernelGGL(row_adam_kernel<4>, dim3((unsigned)adam_blocks), dim3(256), 0, st, param, exp_avg, exp_avg_sq, compact, urow,
                           incl + (n - 1), D, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale, decoupled, factor);
    else
        hipLaunchKernelGGL(row_adam_kernel<1>, dim3((unsigned)adam_blocks), dim3(256), 0, st, param, exp_avg, exp_avg_sq, compact, urow,
                           incl + (n - 1), D, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale, decoupled, factor);
    T4R_LAUNCH_CHECK();
    return 0;
}
