// Workspace plan and host driver shared by the two fused top-k inference heads (item_topk.hip: fp32 table on the fp32 matrix
// cores; item_topk_h16.hip: fp16 / bf16 serving image).  The four steps of a call (item_topk.hip's header) and the host_stats
// bookkeeping are itk_run, once; a head only says how a block of scores is computed and how the collect pass runs.
#pragma once
#include "t4r_common.h"
#include "gumbel_noise.h"
#include "item_filter.h"
#include <algorithm>
#include <math.h>
#include <string>
#include <vector>

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

extern "C" int t4r_topk(void* stream, const float* scores, int N, int V, long ld, int k, float* out_val, long* out_idx);

// Steps 1-4 of one call over the workspace `ws` laid out by `pl`.  The head has three operations, each returning 0 or an error
// code with the message set:
//   head.sample(st, pl, S)                           alpha * scores of the strided sample (items 0, s, 2 s, ...: pl.M of them at
//                                                    s = pl.stride) of every row into S [n_rows, pl.ldS]
//   head.collect(st, thr, thr_ld, count, cand_val, cand_idx, cap)
//                                                    one pass over the table: (score, item) of every score >= thr[row * thr_ld]
//                                                    appended to the row's list (count zeroed here)
//   head.scores(st, r0, n, C, ldv)                   all V scores of rows [r0, r0 + n) into C (row pitch ldv)
// All three must give one (row, item) the same bits.  `name` is the calling entry's: the prefix of the messages of failures in
// here.  host_stats: see t4r_item_topk_f32.
template <class Head>
static int itk_run(const char* name, hipStream_t st, const Plan& pl, void* workspace, int n_rows, int V, int k, float* out_val,
                   long* out_idx, long* host_stats, Head& head) {
    auto fail = [&](const char* what) {
        t4r_set_error((std::string(name) + ": " + what).c_str());
        return -1;
    };
    char* ws = (char*)workspace;
    float* S = (float*)(ws + pl.off_S);
    float* tv = (float*)(ws + pl.off_tv);
    long* ti = (long*)(ws + pl.off_ti);
    int* count = (int*)(ws + pl.off_cnt);
    int* n_flagged = count + n_rows;
    int* flagged = n_flagged + 1;
    float* cand_val = (float*)(ws + pl.off_cand);
    int* cand_idx = (int*)(cand_val + (size_t)n_rows * pl.cap);

    if (hipMemsetAsync(count, 0, sizeof(int) * ((size_t)n_rows + 1), st) != hipSuccess) return fail("memset failed");
    // 1. threshold
    int rc = head.sample(st, pl, S);
    if (rc) return rc;
    rc = t4r_topk(st, S, n_rows, pl.M, pl.ldS, k, tv, ti);
    if (rc) return rc;
    // 2. collect
    rc = head.collect(st, tv + (k - 1), k, count, cand_val, cand_idx, pl.cap);
    if (rc) return rc;
    // 3. select
    rc = t4r_itk_select_launch(st, n_rows, cand_val, cand_idx, count, pl.cap, k, out_val, out_idx, n_flagged, flagged);
    if (rc) return rc;
    // 4. overflow: the one device-to-host read of the call
    int nf = 0;
    if (hipMemcpyAsync(&nf, n_flagged, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail("reading the overflow count failed");
    if (host_stats) { host_stats[1] = pl.M; host_stats[2] = pl.cap; }
    if (host_stats && host_stats[7]) {
        std::vector<int> hc(n_rows);
        if (hipMemcpy(hc.data(), count, sizeof(int) * (size_t)n_rows, hipMemcpyDeviceToHost) != hipSuccess)
            return fail("reading the candidate counts failed");
        long sum = 0, mx = 0;
        for (int c : hc) { sum += c; mx = std::max(mx, (long)c); }
        host_stats[3] = sum; host_stats[4] = mx;
    }
    if (nf > 0) {
        std::vector<int> rows(nf);
        if (hipMemcpy(rows.data(), flagged, sizeof(int) * (size_t)nf, hipMemcpyDeviceToHost) != hipSuccess)
            return fail("reading the overflow rows failed");
        std::sort(rows.begin(), rows.end());          // arrival order of the flags is arbitrary; runs of consecutive rows share a launch
        const long ldv = ((long)V + 63) / 64 * 64;
        const long fit = std::max(1L, (long)((pl.off_x - pl.off_cand) / ((size_t)ldv * 4)));
        float* scores = cand_val;                     // the lists are dead: the select kernel has finished
        for (size_t a = 0; a < rows.size();) {
            size_t b = a + 1;
            while (b < rows.size() && rows[b] == rows[b - 1] + 1 && (long)(b - a) < fit) ++b;
            const int r0 = rows[a], n = (int)(b - a);
            rc = head.scores(st, r0, n, scores, ldv);
            if (rc) return rc;
            rc = t4r_topk(st, scores, n, V, ldv, k, out_val + (long)r0 * k, out_idx + (long)r0 * k);
            if (rc) return rc;
            a = b;
        }
    }
    if (host_stats) host_stats[0] = nf;
    return 0;
}

// scores[r, c] = fp32(scores[r, c] + g(row0 + r, c * item_stride)) in place (item_sample.hip): r < n_rows, c < V, row pitch ld
int t4r_gumbel_add_launch(hipStream_t st, float* scores, int n_rows, int V, long ld, long row0, int item_stride,
                          unsigned long long seed, unsigned long long ctr_hi);

// The sampling form of a head: every score of (row, item) becomes fp32(s + g(row0 + row, item)) -- still a pure function of
// (row, item), so itk_run's four steps stay exact.  The materialised products are the head's own followed by the noise pass;
// the collect pass adds the noise in its epilogue.  All three give one (row, item) the same bits (gumbel_noise.h).
template <class Head>
struct ItkNoisyHead {
    Head head;
    GumbelCfg noise;
    int n_rows, V;

    int sample(hipStream_t st, const Plan& pl, float* S) const {
        const int rc = head.sample(st, pl, S);
        if (rc) return rc;
        return t4r_gumbel_add_launch(st, S, n_rows, pl.M, pl.ldS, noise.row0, pl.stride, noise.seed, noise.ctr_hi);
    }
    int collect(hipStream_t st, const float* thr, long thr_ld, int* count, float* cand_val, int* cand_idx, int cap) const {
        return head.collect(st, thr, thr_ld, count, cand_val, cand_idx, cap, &noise);
    }
    // the signature a plain head's collect has, for ItkFilteredHead: the noise is this head's own, the argument is ignored
    int collect(hipStream_t st, const float* thr, long thr_ld, int* count, float* cand_val, int* cand_idx, int cap,
                const GumbelCfg*, const ItkFilter* filt) const {
        return head.collect(st, thr, thr_ld, count, cand_val, cand_idx, cap, &noise, filt);
    }
    int scores(hipStream_t st, int r0, int n, float* C, long ldv) const {
        const int rc = head.scores(st, r0, n, C, ldv);
        if (rc) return rc;
        return t4r_gumbel_add_launch(st, C, n, V, ldv, noise.row0 + r0, 1, noise.seed, noise.ctr_hi);
    }
};

// The filtered form of a head (Itk32Head, Itk16Head or their noisy forms): every score of (row, item) becomes the score where
// allowed(row, item), -inf otherwise (item_filter.h) -- again a pure function of (row, item), so itk_run's four steps stay exact:
// a finite threshold from the masked sample means k allowed sampled items with those bits exist in the full pass; a -inf
// threshold makes every allowed item a candidate; a row with fewer than k allowed items has fewer than k candidates and takes
// the materialised path like any row the select kernel flags.  The materialised products are the head's own followed by the
// mask; the collect pass tests the filter in its epilogue, so an excluded item never takes a slot of a list.
template <class Head>
struct ItkFilteredHead {
    Head head;
    ItkFilter filt;
    int n_rows, V;

    int sample(hipStream_t st, const Plan& pl, float* S) const {
        const int rc = head.sample(st, pl, S);
        if (rc) return rc;
        return t4r_item_mask_launch(st, S, n_rows, pl.M, pl.ldS, pl.stride, filt);
    }
    int collect(hipStream_t st, const float* thr, long thr_ld, int* count, float* cand_val, int* cand_idx, int cap) const {
        return head.collect(st, thr, thr_ld, count, cand_val, cand_idx, cap, nullptr, &filt);
    }
    int scores(hipStream_t st, int r0, int n, float* C, long ldv) const {
        const int rc = head.scores(st, r0, n, C, ldv);
        if (rc) return rc;
        ItkFilter f = filt;
        if (f.excl) f.excl += (long)r0 * f.ld_excl;
        return t4r_item_mask_launch(st, C, n, V, ldv, 1, f);
    }
};

// a filtered entry: itk_run over the filtered head, then the tail rule -- ids of -inf slots become -1 (t4r_topk's three paths
// do not agree on them) -- as the call's last launch, after the overflow path
template <class Head>
static int itk_run_filtered(const char* name, hipStream_t st, const Plan& pl, void* workspace, int n_rows, int V, int k,
                            float* out_val, long* out_idx, long* host_stats, const Head& base, const ItkFilter& filt) {
    ItkFilteredHead<Head> head = {base, filt, n_rows, V};
    const int rc = itk_run(name, st, pl, workspace, n_rows, V, k, out_val, out_idx, host_stats, head);
    if (rc) return rc;
    return t4r_itk_mark_empty_launch(st, out_val, out_idx, n_rows, k);
}
