// The product of the half-precision serving image, shared by its two consumers (gfx950 only): item_topk_h16.hip (scores and the
// fused top-k head) and item_eval_h16.hip (loss statistics and target ranks in one pass).  What is here IS the arithmetic
// contract of the image: one element is k = 0, 16, 32, ... to ldp, each step one 16-bit MFMA into the same accumulator, whatever
// kernel, launch, tile or row block computes it -- so both files return the same bits for the same (row, item).
#pragma once
#include "t4r_common.h"

#define ITK16_MAX_D 512
#define ITK16_TILE 64          // image rows per workgroup tile

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));

template <int DT>
__device__ __forceinline__ uint32_t round16(float f) {
    if (DT == 3) return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)f);       // v_cvt_f16_f32, RNE
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;                                 // NaN
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;                                       // RNE (overflow rounds to inf)
}

template <int DT>
__device__ __forceinline__ f32x16 mfma16(uint4 a, uint4 b, f32x16 c) {
    if (DT == 3)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, a), __builtin_bit_cast(half8_t, b), c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}

// The image tile of 64 items from item0 on into LDS ([64][chunks + 1] 16-byte slots), by the 256 threads of a workgroup, eight
// 16-byte loads in flight per thread: every load reads a legal address (row clamped into the launch's items) and rows beyond
// them are zeroed on the way to LDS (their columns are masked in the epilogue as well).  Item i of the launch is image row
// i * stride (row pitch ldi elements).  The caller synchronises.
__device__ __forceinline__ void itk16_load_tile(uint4* lds, const uint16_t* img, long ldi, int stride, long item0, int n_items,
                                                int chunks, int tid) {
    const int pitch = chunks + 1;
    const int dr = 256 / chunks, dc = 256 - dr * chunks;  // chunk index + 256 = (row + dr, chunk + dc), carried below
    int tr = tid / chunks, tc = tid - tr * chunks;
    const long last = (long)n_items - 1 - item0;          // last tile row inside the launch's items (>= 0)
    const long rstep = (long)stride * ldi;
    const uint16_t* base = img + item0 * rstep;
    while (tr < ITK16_TILE) {                              // workgroup-divergent only in its last batch
        uint4 v[8];
        int off[8];                                        // LDS slot; -1: beyond the tile; bit 30: zero it
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long rr = min((long)min(tr, ITK16_TILE - 1), last);
            v[u] = *reinterpret_cast<const uint4*>(base + rr * rstep + tc * 8);
            off[u] = tr >= ITK16_TILE ? -1 : ((tr * pitch + tc) | (tr > last ? 1 << 30 : 0));
            tc += dc; tr += dr;
            if (tc >= chunks) { tc -= chunks; ++tr; }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            // first use of the staged registers: keeps the eight loads above in one batch
            asm volatile("" : "+v"(v[u].x), "+v"(v[u].y), "+v"(v[u].z), "+v"(v[u].w));
            const bool z = (off[u] & (1 << 30)) != 0;
            uint4 w;
            w.x = z ? 0u : v[u].x; w.y = z ? 0u : v[u].y; w.z = z ? 0u : v[u].z; w.w = z ? 0u : v[u].w;
            if (off[u] >= 0) lds[off[u] & ~(1 << 30)] = w;
        }
    }
}

// 32 rows of x16 (A fragments from ap, one 16-byte slot per k-step at stride 2) against the 64 items of the LDS tile (B fragments
// from b0p / b1p: items r and 32 + r of the tile): acc[j][e] = sum over k of row (e & 3) + 8 (e >> 2) + 4 h, item 32 j + r.
// k runs 0 .. nk-1 in order into the same two accumulators; the grouping only keeps the next four A fragments in flight.
template <int DT>
__device__ __forceinline__ void itk16_product(const uint4* ap, const uint4* b0p, const uint4* b1p, int nk, f32x16 (&acc)[2]) {
    const int ng = nk >> 2;                                 // groups of four k-steps
#pragma unroll
    for (int e = 0; e < 16; ++e) { acc[0][e] = 0.f; acc[1][e] = 0.f; }
    uint4 a[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = ap[2 * min(u, nk - 1)];
    for (int g = 0; g < ng; ++g) {
        uint4 an[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) an[u] = ap[2 * min(4 * g + 4 + u, nk - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint4 b0 = b0p[2 * (4 * g + u)], b1 = b1p[2 * (4 * g + u)];
            acc[0] = mfma16<DT>(a[u], b0, acc[0]);
            acc[1] = mfma16<DT>(a[u], b1, acc[1]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = an[u];
    }
#pragma unroll
    for (int u = 0; u < 3; ++u) {                           // at most three more steps; a[] holds their fragments already
        if (4 * ng + u < nk) {                              // wave-uniform
            const uint4 b0 = b0p[2 * (4 * ng + u)], b1 = b1p[2 * (4 * ng + u)];
            acc[0] = mfma16<DT>(a[u], b0, acc[0]);
            acc[1] = mfma16<DT>(a[u], b1, acc[1]);
        }
    }
}

}  // namespace

// host side of item_topk_h16.hip, for item_eval_h16.hip
long t4r_itk16_image_ld(long D);
// X fp32 [rows, D] (row pitch ld) -> dst [rows, ldp] in the image's dtype (2 = bf16, 3 = fp16), RNE, pad columns zero
int t4r_itk16_round_rows(hipStream_t st, int dtype, const float* src, long ld, long rows, int D, uint16_t* dst, long ldp);
