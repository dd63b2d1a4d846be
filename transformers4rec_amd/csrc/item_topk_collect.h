// The collect epilogue of the two fused top-k heads, once: gemm_kernel.h (FEAT bit 3, fp32 table) and item_topk_h16.hip (EPI 1,
// fp16 / bf16 image) call it per accumulator element of a 32x32 MFMA block.
#pragma once
#include "item_filter.h"

// A 32-lane half of the wave holds 32 consecutive columns of ONE output row (`row` is uniform over the half, `col` is the
// lane's).  The halves that found candidates (`hit`) reserve their slots in the row's list with ONE returning atomic each
// (first lane of the half) and every candidate stores (v, col) at base + its prefix in the half's ballot; slots beyond `cap`
// are dropped, count[row] keeps counting (the select step flags the row).  Most ballots are empty (a row keeps a few hundred of
// its V scores): those cost a compare and a wave-uniform branch.  Every lane of the wave must call it.
__device__ __forceinline__ void itk_collect(bool hit, float v, int col, int row, int lane, int* count, float* cand_val,
                                            int* cand_idx, int cap) {
    const unsigned long long m = __ballot(hit);
    if (m == 0) return;                                     // wave-uniform
    const int r = lane & 31, h = lane >> 5;                 // lane r of half h
    const unsigned mh = (unsigned)(h ? (m >> 32) : (m & 0xffffffffull));
    int base = 0;
    if (r == 0 && mh) base = atomicAdd(count + row, __popc(mh));
    base = __shfl(base, lane & 32, 64);
    const int slot = base + __popc(mh & ((1u << r) - 1u));
    if (hit && slot < cap) {
        cand_val[(long)row * cap + slot] = v;
        cand_idx[(long)row * cap + slot] = col;
    }
}

// itk_collect under an item filter (item_filter.h).  The caller has already folded the allow BIT of the lane's column into
// `hit` (one word per half, loaded outside the row loop), so a dense catalogue filter keeps the ballots empty; the row's
// exclusion LIST is searched only here, behind the rare non-empty ballot, and a second ballot drops what it found: an excluded
// item never takes a slot.
__device__ __forceinline__ void itk_collect_filtered(bool hit, float v, int col, int row, int lane, int* count, float* cand_val,
                                                     int* cand_idx, int cap, const ItkFilter& f) {
    if (__ballot(hit) == 0) return;                         // wave-uniform
    if (hit && itk_row_listed(f, row, col)) hit = false;
    itk_collect(hit, v, col, row, lane, count, cand_val, cand_idx, cap);
}
