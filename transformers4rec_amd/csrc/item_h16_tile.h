// The product of the half-precision serving image, shared by its two consumers (gfx950 only): item_topk_h16.hip (scores and the
// fused top-k head) and item_eval_h16.hip (loss statistics and target ranks in one pass).  What is here IS the arithmetic
// contract of the image: one element is k = 0, 16, 32, ... to ldp, each step one 16-bit MFMA into the same accumulator, whatever
// kernel, launch, tile or row block computes it -- so both files return the same bits for the same (row, item).
// The host side of the contract is here as well, once for every entry that takes an image: its pitch, the supported widths, the
// argument check, the tile's LDS size and the dispatch on the image's dtype.
#pragma once
#include "t4r_common.h"
#include <type_traits>

#define ITK16_MAX_D 512
#define ITK16_TILE 64          // image rows per workgroup tile

// row pitch (elements) of an image of width D: D rounded up to the k step (16 elements = 32 bytes)
static inline long itk16_image_ld(long D) { return (D + 15) / 16 * 16; }
static inline bool itk16_supported(int D) { return D >= 1 && D <= ITK16_MAX_D; }
// dynamic LDS of a workgroup's tile: [ITK16_TILE][ldp / 8 + 1] 16-byte slots (ldp: k extent, a multiple of 16)
static inline size_t itk16_lds_bytes(int ldp) { return (size_t)ITK16_TILE * ((size_t)(ldp >> 3) + 1) * 16; }

// f(std::integral_constant<int, DT>) with DT the image's dtype code: 2 = bf16, 3 = fp16 (the caller has checked it)
template <class F>
static inline int itk16_dispatch(int dtype, F&& f) {
    return dtype == 3 ? f(std::integral_constant<int, 3>()) : f(std::integral_constant<int, 2>());
}

// the image arguments (dtype, image, ldp, D) of the entry `name`
#define ITK16_CHECK_IMAGE(name)                                                                                                     \
    T4R_CHECK_ARG(dtype == 2 || dtype == 3, name ": dtype is 2 (bf16) or 3 (fp16), the codes of T4R_GEMM_PREC");                    \
    T4R_CHECK_ARG(ldp >= itk16_image_ld(D) && ldp % 8 == 0 && (uintptr_t)image % 16 == 0,                                           \
                  name ": image rows must be 16-byte aligned with pitch >= t4r_item_table_image_ld(D)")

// X fp32 [rows, D] (row pitch ld) -> dst [rows, ldp] in the image's dtype, RNE, pad columns zero (item_topk_h16.hip): the pack of
// the table and the rounding of x of every entry
int t4r_itk16_round_rows(hipStream_t st, int dtype, const float* src, long ld, long rows, int D, uint16_t* dst, long ldp);

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

// C/D layout of the 32x32 MFMA: accumulator element e of a lane in half h (= lane >> 5) belongs to this row of the block
__device__ __forceinline__ int itk16_acc_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

// 32 rows of x16 (A fragments from ap, one 16-byte slot per k-step at stride 2) against the 64 items of the LDS tile (B fragments
// from b0p / b1p: items r and 32 + r of the tile): acc[j][e] = sum over k of row itk16_acc_row(e, h), item 32 j + r.
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
