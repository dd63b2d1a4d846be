// Workspace plan and the select step shared by the two fused top-k inference heads (item_topk.hip: fp32 table on the fp32
// matrix cores; item_topk_h16.hip: fp16 / bf16 serving image).
#pragma once
#include "t4r_common.h"
#include <algorithm>
#include <math.h>

#define ITK_MAX_K 256
#define ITK_LDS_CAP 2048       // candidates >= t1 held in LDS by the select kernel (t4r_topk's own list size)

// Sizes of one call, from (V, k) alone.  The number of scores >= the k-th largest of M sampled ones is about k V / M on
// average (the k-th of M order statistics), with a Gamma(k)-like spread: for k >= 10 its maximum over rows stayed below
// 2.6 x the mean (CPU simulation at V = 100 001, Gaussian and popularity-skewed tables), for small k the tail is long
// (k = 1: exponential).  cap = mean * max(4, (k + 6 sqrt(k) + 16) / k) keeps the overflow probability of a row below ~1e-9
// for every k.  M balances the two buffers that grow against each other (S: 4 M bytes per row, lists: 8 cap bytes per row).
struct Plan {
    int M, stride, ldS, cap;
    size_t off_wsamp, off_S, off_tv, off_ti, off_cnt, off_cand, off_x, total;
};

static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// samp_row_bytes: bytes of one gathered sample row (0: the caller scores the sample in place); x_bytes: a region of the caller's
// own behind the lists (the 16-bit image of x; 0: none)
static inline Plan make_plan(long n_rows, long V, int k, size_t samp_row_bytes, size_t x_bytes) {
    Plan p;
    const double f = std::max(4.0, (k + 6.0 * sqrt((double)k) + 16.0) / k);
    long M = (long)ceil(sqrt(2.0 * f * (double)k * (double)V));
    M = std::max(M, 1024L);
    M = (M + 63) / 64 * 64;
    if (M >= V) { M = V; p.stride = 1; }
    else p.stride = (int)(V / M);                 // (M - 1) * stride < V
    p.M = (int)M;
    p.ldS = (int)((M + 3) / 4 * 4);
    const double mean = (double)k * (double)V / (double)M;
    long cap = (long)ceil(mean * f);
    cap = std::max(cap, 2048L);
    cap = (cap + 63) / 64 * 64;
    p.cap = (int)std::min(cap, (V + 3) / 4 * 4);  // a row never has more than V candidates
    size_t o = 0;
    p.off_wsamp = o; o += align256((size_t)M * samp_row_bytes);
    p.off_S = o;     o += align256((size_t)n_rows * p.ldS * 4);
    p.off_tv = o;    o += align256((size_t)n_rows * k * 4);
    p.off_ti = o;    o += align256((size_t)n_rows * k * 8);
    p.off_cnt = o;   o += align256((size_t)(2 * n_rows + 1) * 4);      // count[N] | n_flagged | flagged[N]
    p.off_cand = o;
    // the candidate region doubles as the score buffer of the overflow path: at least one padded row of scores
    const size_t row_scores = (size_t)((V + 63) / 64 * 64) * 4;
    o += align256(std::max((size_t)n_rows * p.cap * 8, row_scores));
    p.off_x = o;     o += align256(x_bytes);
    p.total = o;
    return p;
}

// step 3 (item_topk.hip): one workgroup per row ranks the row's candidate list, flags the rows that overflowed
int t4r_itk_select_launch(hipStream_t st, int n_rows, const float* cand_val, const int* cand_idx, const int* count, int cap, int k,
                          float* out_val, long* out_idx, int* n_flagged, int* flagged);
