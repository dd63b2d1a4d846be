// Item filters of the fused top-k / sampling heads (include/t4r_hip_filter.h): which items a row may return.
//
// A filter has two optional parts:
//   allow_bits   a catalogue filter shared by all rows: bit (v & 31) of 32-bit word (v >> 5) is set where item v may be
//                returned; 2 * ceil(V / 64) words (one 64-item collect tile's worth, so a lane of an edge tile reads a legal
//                word), bits at and beyond V zero.  Null: everything is allowed.
//   excl         a per-row exclusion list (the session's seen items): [n_rows, n_excl] int64, row pitch ld_excl >= n_excl,
//                0 <= n_excl <= ITK_MAX_EXCL, every row in non-decreasing order.  Entries outside [0, V) are ignored (-1 pads),
//                duplicates are fine.  Null or n_excl = 0: no list.
//                Rows that are NOT sorted are memory-safe (every search stays inside the row); for them it is unspecified
//                which of the listed items are excluded.
// allowed(row, v) = (no bits or bit v set) and v not in the row's list.  The filtered score is s where allowed, -inf otherwise:
// a pure function of (row, item), so itk_run's four steps (item_topk_plan.h) stay exact over it.
#pragma once
#include "t4r_common.h"

#define ITK_MAX_EXCL 1024

struct ItkFilter {
    const unsigned* allow_bits;
    const long* excl;
    int n_excl;
    long ld_excl;
};

// the allow word of the 32 items v0 .. v0 + 31 (v0 a multiple of 32): all ones without a bit array
__device__ __forceinline__ unsigned itk_allow_word(const unsigned* __restrict__ allow_bits, long v0) {
    return allow_bits ? allow_bits[v0 >> 5] : 0xffffffffu;
}

__device__ __forceinline__ bool itk_allowed_bit(const unsigned* __restrict__ allow_bits, long v) {
    return (itk_allow_word(allow_bits, v & ~31L) >> (v & 31)) & 1u;
}

// is v in list[0 .. n)?  Binary search for the first entry >= v; lo and hi never leave [0, n] whatever the order of the list.
__device__ __forceinline__ bool itk_listed(const long* __restrict__ list, int n, long v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && list[lo] == v;
}

__device__ __forceinline__ bool itk_row_listed(const ItkFilter& f, long row, long v) {
    return f.excl && f.n_excl > 0 && itk_listed(f.excl + row * f.ld_excl, f.n_excl, v);
}

__device__ __forceinline__ bool itk_allowed(const ItkFilter& f, long row, long v) {
    return itk_allowed_bit(f.allow_bits, v) && !itk_row_listed(f, row, v);
}

// in place on scores [n_rows, >= V] (pitch ld): column c (item c * item_stride) of row r becomes -inf where the item is not
// allowed; `f.excl` is the list of the launch's first row (item_filter.hip)
int t4r_item_mask_launch(hipStream_t st, float* scores, int n_rows, int V, long ld, int item_stride, const ItkFilter& f);
// the tail rule: idx[r, j] = -1 where val[r, j] == -inf, over [n_rows, k] (item_filter.hip)
int t4r_itk_mark_empty_launch(hipStream_t st, const float* val, long* idx, int n_rows, int k);
// the argument checks every entry that takes a filter shares; 0 or -1 with the message set (prefix `name`)
int t4r_item_filter_check(const char* name, const unsigned* allow_bits, const long* excl, int n_excl, long ld_excl);
