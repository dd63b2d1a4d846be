// Gumbel noise of the sampling heads (csrc/item_sample.hip; the noisy collect epilogues of gemm_kernel.h and item_topk_h16.hip).
//
// The draw of (row, item) under (seed, ctr_hi) is a pure function of those four numbers:
//   block = Philox4x32-10(key = seed, counter words c0 = item, c1 = row >> 2, (c2, c3) = ctr_hi)
//   w     = word (row & 3) of the block
//   u     = ((w >> 9) + 0.5) * 2^-23          exact in fp32, in [2^-24, 1 - 2^-24]: no epsilons
//   g     = -log(-log u)                       in [-2.81, 16.64]
// and the perturbed score is fp32(s + g): ONE add with one rounding, never contracted with the multiplication that made s.
// Four consecutive rows of one item share a block: a lane of a 32x32 accumulator fragment holds exactly such a run (row base a
// multiple of 4), so the collect epilogues pay one block function per four scores and need no quad transpose.  Nothing here
// depends on n_rows, V, a pitch or a tile: every kernel that perturbs a score of (row, item) produces the same bits.
// Both logarithms are the accurate ones (<= 1 ulp): -log u spans 6e-8 .. 16.6, where v_log_f32's absolute error would be the
// whole value at the small end.
#pragma once
#include "t4r_common.h"

struct GumbelCfg {
    unsigned long long seed, ctr_hi;
    long row0;                      // row r of the launch is row row0 + r of the stream
};

__device__ __forceinline__ float gumbel_of_word(uint32_t w) {
    const float u = ((float)(w >> 9) + 0.5f) * (1.0f / 8388608.0f);
    return -logf(-logf(u));
}
__device__ __forceinline__ uint4 gumbel_block(const GumbelCfg& c, uint32_t rowq, uint32_t item) {
    const Philox rng(c.seed);
    return rng(((uint64_t)rowq << 32) | item, c.ctr_hi);
}
// the single rounding of the contract: the add carries no contraction licence, whatever produced s
__device__ __forceinline__ float gumbel_perturb(float s, float g) {
#pragma clang fp contract(off)
    return s + g;
}
// noise of the four stream rows 4 rowq .. 4 rowq + 3 of `item`
__device__ __forceinline__ void gumbel4(const GumbelCfg& c, uint32_t rowq, uint32_t item, float (&g)[4]) {
    const uint4 w = gumbel_block(c, rowq, item);
    g[0] = gumbel_of_word(w.x); g[1] = gumbel_of_word(w.y); g[2] = gumbel_of_word(w.z); g[3] = gumbel_of_word(w.w);
}
// noise of the launch's rows local .. local + 3 (local % 4 == 0) of `item`.  row0 % 4 == 0: one block; otherwise the run
// straddles two blocks (wave-uniform: row0 is the launch's)
__device__ __forceinline__ void gumbel_quad(const GumbelCfg& c, int local, uint32_t item, float (&g)[4]) {
    const int a = (int)(c.row0 & 3);
    const uint32_t q = (uint32_t)(((long)local + c.row0) >> 2);
    const uint4 w0 = gumbel_block(c, q, item);
    if (a == 0) {
        g[0] = gumbel_of_word(w0.x); g[1] = gumbel_of_word(w0.y); g[2] = gumbel_of_word(w0.z); g[3] = gumbel_of_word(w0.w);
        return;
    }
    const uint4 w1 = gumbel_block(c, q + 1, item);
    const uint32_t w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t s = a == 1 ? w[1 + e] : (a == 2 ? w[2 + e] : w[3 + e]);
        g[e] = gumbel_of_word(s);
    }
}
