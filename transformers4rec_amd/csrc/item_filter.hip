// Item filters over MATERIALISED scores and the small kernels around the filtered heads (gfx950 only): the entries of
// include/t4r_hip_filter.h that are not a head.  The fused forms -- the same predicate (item_filter.h) inside the collect pass of
// the two top-k heads -- are FEAT bit 5 of gemm_kernel.h and EPI 3 / 4 of item_topk_h16.hip.
//
// Replaces the `scores[mask] = -inf` a caller of the reference's inference writes on the full scores it is handed
// (transformers4rec/torch/model/prediction_task.py:452-470) before torch.topk: seen items of the session, catalogue filters.
//
//   item_mask_kernel         in place on scores [n_rows, >= V] (pitch ld): column c stands for item c * item_stride; disallowed
//                            columns become -inf whatever they held.  It never READS the scores: the bit part is one thread per
//                            column that loads its allow word and, where the bit is clear, stores -inf down a group of 16 rows
//                            (a dense filter stores whole 256-byte row segments, a sparse one almost nothing); the list part is
//                            one thread per list entry and one store.  Allowed columns and pad columns V .. ld - 1 are not touched.
//   item_allow_pack_kernel   [V] bytes (non-zero = allowed) -> the bit words, one ballot per 64 items; the pad bits of the last
//                            pair of words are written as zero.
//   itk_mark_empty_kernel    the tail rule over [n_rows, k]: id = -1 where the value is -inf.
#include "item_filter.h"
#include "t4r_common.h"
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string>

#define ITEM_MASK_ROWS 16

namespace {

// workgroup b of a row group: b < col_blocks is the bit part of columns 256 b .., b == col_blocks the list part
__global__ __launch_bounds__(256) void item_mask_kernel(float* __restrict__ scores, int n_rows, int V, long ld, int item_stride,
                                                         int col_blocks, int blocks_per_group, ItkFilter f) {
    const int b = (int)(blockIdx.x % blocks_per_group);
    const int r0 = (int)(blockIdx.x / blocks_per_group) * ITEM_MASK_ROWS;
    const int nr = min(ITEM_MASK_ROWS, n_rows - r0);
    if (b < col_blocks) {
        const int c = b * 256 + threadIdx.x;
        if (c >= V || itk_allowed_bit(f.allow_bits, (long)c * item_stride)) return;
        float* s = scores + (long)r0 * ld + c;
        for (int r = 0; r < nr; ++r) s[(long)r * ld] = -INFINITY;
        return;
    }
    for (int i = threadIdx.x; i < nr * f.n_excl; i += 256) {
        const int r = r0 + i / f.n_excl;
        const long v = f.excl[(long)r * f.ld_excl + i % f.n_excl];
        if (v < 0 || v % item_stride != 0) continue;
        const long c = v / item_stride;
        if (c < V) scores[(long)r * ld + c] = -INFINITY;
    }
}

__global__ __launch_bounds__(256) void item_allow_pack_kernel(const unsigned char* __restrict__ allow, int V, int groups,
                                                               unsigned* __restrict__ bits) {
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= groups) return;                                 // wave-uniform
    const long v = (long)g * 64 + lane;
    const unsigned long long m = __ballot(v < V && allow[min(v, (long)V - 1)] != 0);
    if (lane == 0) {
        bits[2 * g] = (unsigned)(m & 0xffffffffull);
        bits[2 * g + 1] = (unsigned)(m >> 32);
    }
}

__global__ __launch_bounds__(256) void itk_mark_empty_kernel(const float* __restrict__ val, long* __restrict__ idx, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && val[i] == -INFINITY) idx[i] = -1;
}

}  // namespace

int t4r_item_filter_check(const char* name, const unsigned* allow_bits, const long* excl, int n_excl, long ld_excl) {
    const char* what = nullptr;
    if ((uintptr_t)allow_bits % 4 != 0) what = "allow_bits must be 4-byte aligned";
    else if (n_excl < 0 || n_excl > ITK_MAX_EXCL) what = "0 <= n_excl <= 1024";
    else if (n_excl > 0 && !excl) what = "excl is null with n_excl > 0";
    else if (n_excl > 0 && ld_excl < n_excl) what = "ld_excl below n_excl";
    else if ((uintptr_t)excl % 8 != 0) what = "excl must be 8-byte aligned";
    if (!what) return 0;
    t4r_set_error((std::string(name) + ": " + what).c_str());
    return -1;
}

int t4r_item_mask_launch(hipStream_t st, float* scores, int n_rows, int V, long ld, int item_stride, const ItkFilter& f) {
    if (n_rows <= 0 || V <= 0) return 0;
    const bool list = f.excl && f.n_excl > 0;
    const int col_blocks = f.allow_bits ? (V + 255) / 256 : 0;
    const int per_group = col_blocks + (list ? 1 : 0);
    if (per_group == 0) return 0;
    const long blocks = (((long)n_rows + ITEM_MASK_ROWS - 1) / ITEM_MASK_ROWS) * per_group;
    T4R_CHECK_ARG(blocks <= INT_MAX, "item_mask: n_rows * V beyond one launch (2^31 workgroups of 16 rows x 256 columns)");
    hipLaunchKernelGGL(item_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, st, scores, n_rows, V, ld, item_stride, col_blocks,
                       per_group, f);
    T4R_LAUNCH_CHECK();
    return 0;
}

int t4r_itk_mark_empty_launch(hipStream_t st, const float* val, long* idx, int n_rows, int k) {
    const long n = (long)n_rows * k;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(itk_mark_empty_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, val, idx, n);
    T4R_LAUNCH_CHECK();
    return 0;
}

extern "C" long t4r_item_allow_words(int V) { return V > 0 ? 2 * (((long)V + 63) / 64) : 0; }

extern "C" int t4r_item_allow_pack(void* stream, const unsigned char* allow, int V, unsigned* bits) {
    if (V == 0) return 0;
    T4R_CHECK_ARG(V > 0 && allow && bits, "item_allow_pack: bad arguments");
    T4R_CHECK_ARG((uintptr_t)bits % 4 == 0, "item_allow_pack: bits must be 4-byte aligned");
    const int groups = (V + 63) / 64;
    hipLaunchKernelGGL(item_allow_pack_kernel, dim3((unsigned)((groups + 3) / 4)), dim3(256), 0, (hipStream_t)stream, allow, V,
                       groups, bits);
    T4R_LAUNCH_CHECK();
    return 0;
}

extern "C" int t4r_item_mask_f32(void* stream, float* scores, int n_rows, int V, long ld, int item_stride,
                                 const unsigned* allow_bits, const long* excl, int n_excl, long ld_excl) {
    if (n_rows == 0 || V == 0) return 0;
    T4R_CHECK_ARG(n_rows > 0 && V > 0 && scores, "item_mask: bad arguments");
    T4R_CHECK_ARG(ld >= V, "item_mask: row pitch below V");
    T4R_CHECK_ARG(item_stride >= 1 && (long)(V - 1) * item_stride < (1L << 31), "item_mask: items are 0 .. 2^31 - 1, item_stride >= 1");
    if (t4r_item_filter_check("item_mask", allow_bits, excl, n_excl, ld_excl)) return -1;
    return t4r_item_mask_launch((hipStream_t)stream, scores, n_rows, V, ld, item_stride, ItkFilter{allow_bits, excl, n_excl, ld_excl});
}
