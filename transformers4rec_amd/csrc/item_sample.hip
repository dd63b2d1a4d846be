// Gumbel noise over MATERIALISED scores (gfx950 only): the two kernels of include/t4r_hip_sampling.h that take an [n_rows, V]
// fp32 matrix.  The fused forms -- the same noise inside the collect pass of the two top-k heads -- are the FEAT 24 epilogue of
// gemm_kernel.h and EPI 2 of item_topk_h16.hip; the noise itself is gumbel_noise.h, once.
//
// Replaces the draw of the reference's replacement-token masking (transformers4rec/torch/masking.py:851-870, sample_from_softmax:
// torch.rand, two logs, add, argmax over [N_m, V]), and is the k > 1 generalisation (Gumbel top-k = k draws without replacement
// in proportion to softmax(scores)) that t4r_item_sample_f32 / _h16 serve.
//
//   gumbel_add_kernel      scores[r, c] = fp32(scores[r, c] + g(row0 + r, c * item_stride)), in place.  One thread per (aligned
//                          quad of stream rows, column): one Philox block serves the four rows; columns are the fast index, so
//                          each of the four row accesses of a wave is one contiguous 256-byte segment.  Pad columns c >= V are
//                          not touched.
//   gumbel_argmax_kernel   (max over c of fp32(scores[r, c] + g), its c) per row, ties to the lower c, without writing the
//                          perturbed scores: one workgroup per quad of stream rows walks the columns once.  Bit for bit
//                          t4r_topk(k = 1) of gumbel_add's output: the same fp32 values, the same order rule.
#include "gumbel_noise.h"
#include <limits.h>
#include <math.h>

int t4r_gumbel_add_launch(hipStream_t st, float* scores, int n_rows, int V, long ld, long row0, int item_stride,
                          unsigned long long seed, unsigned long long ctr_hi);

namespace {

__global__ __launch_bounds__(256) void gumbel_add_kernel(float* __restrict__ scores, int n_rows, int V, long ld, int item_stride,
                                                          int col_blocks, GumbelCfg cfg) {
    const long q = (cfg.row0 >> 2) + blockIdx.x / col_blocks;          // quad of stream rows 4 q .. 4 q + 3
    const int c = (int)(blockIdx.x % col_blocks) * 256 + threadIdx.x;
    if (c >= V) return;
    float g[4];
    gumbel4(cfg, (uint32_t)q, (uint32_t)c * (uint32_t)item_stride, g);
    const long r0 = (q << 2) - cfg.row0;                               // the launch's row of the quad's first word (may be < 0)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const long r = r0 + e;
        if (r < 0 || r >= n_rows) continue;                            // workgroup-uniform
        float* s = scores + r * ld + c;
        *s = gumbel_perturb(*s, g[e]);
    }
}

// (value desc, index asc): does (v, i) come before (bv, bi)?
__device__ __forceinline__ bool gumbel_before(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__global__ __launch_bounds__(256) void gumbel_argmax_kernel(const float* __restrict__ scores, int n_rows, int V, long ld,
                                                             GumbelCfg cfg, float* __restrict__ out_val,
                                                             long* __restrict__ out_idx) {
    __shared__ float sv[4][4];
    __shared__ int si[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long q = (cfg.row0 >> 2) + blockIdx.x;
    const long r0 = (q << 2) - cfg.row0;
    float bv[4];
    int bi[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { bv[e] = -INFINITY; bi[e] = 0; }
    for (int c = tid; c < V; c += 256) {
        float g[4];
        gumbel4(cfg, (uint32_t)q, (uint32_t)c, g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long r = r0 + e;
            if (r < 0 || r >= n_rows) continue;                        // workgroup-uniform
            const float v = gumbel_perturb(scores[r * ld + c], g[e]);
            if (v > bv[e]) { bv[e] = v; bi[e] = c; }                   // c ascends: the first of equal values stays
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv[e], o, 64);
            const int oi = __shfl_xor(bi[e], o, 64);
            if (gumbel_before(ov, oi, bv[e], bi[e])) { bv[e] = ov; bi[e] = oi; }
        }
        if (lane == 0) { sv[wave][e] = bv[e]; si[wave][e] = bi[e]; }
    }
    __syncthreads();
    if (tid < 4) {
        const long r = r0 + tid;
        if (r < 0 || r >= n_rows) return;
        float v = sv[0][tid];
        int i = si[0][tid];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (gumbel_before(sv[w][tid], si[w][tid], v, i)) { v = sv[w][tid]; i = si[w][tid]; }
        out_val[r] = v;
        out_idx[r] = i;
    }
}

// quads of stream rows the launch's rows row0 .. row0 + n_rows - 1 touch
inline long gumbel_quads(long row0, int n_rows) { return ((row0 + n_rows - 1) >> 2) - (row0 >> 2) + 1; }

}  // namespace

int t4r_gumbel_add_launch(hipStream_t st, float* scores, int n_rows, int V, long ld, long row0, int item_stride,
                          unsigned long long seed, unsigned long long ctr_hi) {
    if (n_rows <= 0 || V <= 0) return 0;
    const int col_blocks = (V + 255) / 256;
    const long blocks = gumbel_quads(row0, n_rows) * col_blocks;
    T4R_CHECK_ARG(blocks <= INT_MAX, "gumbel_add: n_rows * V beyond one launch (2^31 workgroups of 4 rows x 256 columns)");
    const GumbelCfg cfg = {seed, ctr_hi, row0};
    hipLaunchKernelGGL(gumbel_add_kernel, dim3((unsigned)blocks), dim3(256), 0, st, scores, n_rows, V, ld, item_stride, col_blocks,
                       cfg);
    T4R_LAUNCH_CHECK();
    return 0;
}

extern "C" int t4r_gumbel_add_f32(void* stream, float* scores, int n_rows, int V, long ld, long row0, int item_stride,
                                  unsigned long long seed, unsigned long long ctr_hi) {
    if (n_rows == 0 || V == 0) return 0;
    T4R_CHECK_ARG(n_rows > 0 && V > 0 && scores, "gumbel_add: bad arguments");
    T4R_CHECK_ARG(ld >= V, "gumbel_add: row pitch below V");
    T4R_CHECK_ARG(row0 >= 0 && row0 + n_rows <= (1L << 34), "gumbel_add: rows of the stream are 0 .. 2^34 - 1");
    T4R_CHECK_ARG(item_stride >= 1 && (long)(V - 1) * item_stride < (1L << 32), "gumbel_add: items are 0 .. 2^32 - 1, item_stride >= 1");
    return t4r_gumbel_add_launch((hipStream_t)stream, scores, n_rows, V, ld, row0, item_stride, seed, ctr_hi);
}

extern "C" int t4r_gumbel_argmax_f32(void* stream, const float* scores, int n_rows, int V, long ld, long row0,
                                     unsigned long long seed, unsigned long long ctr_hi, float* out_val, long* out_idx) {
    if (n_rows == 0) return 0;
    T4R_CHECK_ARG(n_rows > 0 && V > 0 && scores && out_val && out_idx, "gumbel_argmax: bad arguments");
    T4R_CHECK_ARG(ld >= V, "gumbel_argmax: row pitch below V");
    T4R_CHECK_ARG(row0 >= 0 && row0 + n_rows <= (1L << 34), "gumbel_argmax: rows of the stream are 0 .. 2^34 - 1");
    const GumbelCfg cfg = {seed, ctr_hi, row0};
    hipLaunchKernelGGL(gumbel_argmax_kernel, dim3((unsigned)gumbel_quads(row0, n_rows)), dim3(256), 0, (hipStream_t)stream, scores,
                       n_rows, V, ld, cfg, out_val, out_idx);
    T4R_LAUNCH_CHECK();
    return 0;
}
