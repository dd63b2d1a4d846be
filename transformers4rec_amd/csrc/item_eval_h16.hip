// Evaluation head over a half-precision SERVING IMAGE of the item table (gfx950 only): loss statistics and target ranks in ONE
// pass over the image, without the [N, V] scores.
//
// Replaces, for a model evaluated under fp16=True / bf16=True (autocast, transformers4rec/torch/trainer.py:363-367), the chain
// logits (model/prediction_task.py:430) -> log_softmax + CrossEntropyLoss (label smoothing) for the loss, and -> torch.topk + the
// [N, V] one-hot of ranking_metric.py:52-59 for the ranking metrics.  Per label row n, with s[n, v] the bits t4r_item_scores_h16
// returns (item_h16_tile.h: x rounded once, one 16-bit MFMA per k-step into one accumulator, then * alpha):
//
//   target[n]    = s[n, labels[n]]                                            bit for bit
//   rank[n]      = #{v : s[n,v] > target[n] or (s[n,v] == target[n] and v < labels[n])}      (the rule of t4r_rank_of_target_f32)
//   lse[n]       = log sum_v exp(s[n,v])          fp32, running maximum
//   score_sum[n] = sum_v s[n,v]                   fp32 (label smoothing: loss = (1-eps)(lse - target) + eps (lse - score_sum / V))
//
// Kernels
//   itev16_target_kernel   one wave per 32 rows: A = the rows of x16, B = the image rows of their labels read straight from the
//                          image, the k loop of the main pass on ONE accumulator; the diagonal of the 32 x 32 block is target.
//                          (An element's bits do not depend on where in a block it sits: the contract item_topk_h16.hip rests on.)
//                          It also initialises rank: 0, or V for a label outside [0, V) (target NaN: nothing compares as a hit).
//   itev16_kernel          the item-tile-stationary product of itk16_kernel.  A workgroup walks a contiguous run of G tiles; its
//                          wave w revisits rows 32 w + 128 i in every tile.  Epilogue per 32 x 64 block: a row's 64 scores sit in
//                          the 32 lanes of one half (two per lane).  Rank hits: two ballots, one integer atomicAdd by the half's
//                          first lane where the count is non-zero.  (max, sum exp, sum) are reduced over each 16-lane row with
//                          four DPP steps, the lane e of the row keeps the result of accumulator element e, and after the 16
//                          elements the two 16-lane rows are merged once and lanes 0..15 of each half fold the block into the
//                          row's running (max, sumexp, sum) -- 16 bytes in this workgroup's own slice of the workspace, no atomics.
//   itev16_finalise_kernel merges the groups' partials of a row in a fixed order (64 interleaved chains, then a pairwise tree) and
//                          writes lse and score_sum.
//
// Reproducibility: G and the number of groups are functions of V alone; every reduction has a fixed order and touches one row's
// scores only; the only atomics are integer.  So a row's four outputs do not depend on n_rows, on the other rows or on the call.
// NaN: a NaN score reaches lse through the exponentials (this file is compiled with NaNs honoured).
//
// Longest chain of additions-and-rescales behind one lse: 1 (two scores of a lane) + 4 (DPP) + 1 (the two 16-lane rows) + G (tiles
// of the group) + ceil(groups / 64) + 6 (finalise).  G = ceil(tiles / 2048) capped at 64: 64 + 39 + 12 = 115 at V = 10 000 001;
// it passes 150 only beyond V = 19 M (one more step per 4096 items from there).
#include "item_h16_tile.h"
#include <algorithm>
#include <math.h>

#define ITEV16_GROUPS 2048     // target number of workgroups (each keeps n_rows x 16 bytes of partials)
#define ITEV16_MAX_G 64        // tiles per workgroup at most: bounds the sequential part of the lse chain

namespace {

struct Itev16Params {
    int n_rows, V, ldp;             // ldp: k extent (multiple of 16) = pitch of x16
    const uint16_t* x16;            // [n_rows, ldp]
    const uint16_t* img; long ldi;
    float alpha;
    const long* labels;
    float* target;
    int* rank;
    float4* part;                   // [groups, n_rows] (max, sumexp, sum, -)
    int G; long tiles; int groups;
    float* lse; float* score_sum;
};

template <int DT>
__global__ __launch_bounds__(64) void itev16_target_kernel(Itev16Params p) {
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int rb = blockIdx.x * 32;
    const int row = min(rb + r, p.n_rows - 1);
    const long lab = p.labels[row];
    const bool bad = lab < 0 || lab >= p.V;
    const uint4* ap = reinterpret_cast<const uint4*>(p.x16 + (long)row * p.ldp) + h;
    const uint4* bp = reinterpret_cast<const uint4*>(p.img + (bad ? 0 : lab) * p.ldi) + h;
    const int nk = p.ldp >> 4;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    for (int s = 0; s < nk; ++s) acc = mfma16<DT>(ap[2 * s], bp[2 * s], acc);
    // element e of lane (r, h) is row itk16_acc_row(e, h), column r: the diagonal entry of column r sits in half (r >> 2) & 1
    const int ed = (r & 3) + 4 * (r >> 3);
    float d = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) d = e == ed ? acc[e] : d;
    if (h == ((r >> 2) & 1) && rb + r < p.n_rows) {
        p.target[rb + r] = bad ? __builtin_nanf("") : p.alpha * d;
        p.rank[rb + r] = bad ? p.V : 0;
    }
}

template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// all-reduce over the 16 lanes of a DPP row: lane ^ 1, lane ^ 2 (quad permutes), then the mirrored half row and the mirrored row
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, dpp<0xB1>(v)); v = fmaxf(v, dpp<0x4E>(v)); v = fmaxf(v, dpp<0x141>(v)); v = fmaxf(v, dpp<0x140>(v));
    return v;
}
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp<0xB1>(v); v += dpp<0x4E>(v); v += dpp<0x141>(v); v += dpp<0x140>(v);
    return v;
}

// (m, s) <- (m, s) (+) (m2, s2) for sums of exponentials kept as s * exp(m).  m == -inf with s == 0 is the empty sum; the factor
// of the side that holds the maximum is exactly 1, so equal maxima (and two empty sums) add without a rounding of their own.
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
    const float nm = fmaxf(m, m2);
    const float f1 = m == nm ? 1.f : __expf(m - nm), f2 = m2 == nm ? 1.f : __expf(m2 - nm);
    s = s * f1 + s2 * f2;
    m = nm;
}

template <int DT>
__global__ __launch_bounds__(256) void itev16_kernel(Itev16Params p) {
    extern __shared__ uint4 itev16_lds[];                   // [64][chunks + 1] 16-byte slots
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunks = p.ldp >> 3, pitch = chunks + 1;
    const int r = lane & 31, h = lane >> 5;
    const uint4* b0p = itev16_lds + r * pitch + h;
    const uint4* b1p = itev16_lds + (32 + r) * pitch + h;
    const int nk = p.ldp >> 4;
    const float alpha = p.alpha;
    const float ninf = -__builtin_inff();
    const long t0 = (long)blockIdx.x * p.G, t1 = min(t0 + p.G, p.tiles);
    float4* part = p.part + (long)blockIdx.x * p.n_rows;
    const int krow = itk16_acc_row(r & 15, h);              // the row (within the block) whose statistics this lane keeps
    for (long t = t0; t < t1; ++t) {
        const long item0 = t * ITK16_TILE;
        if (t > t0) __syncthreads();                        // every wave is done with the previous tile
        itk16_load_tile(itev16_lds, p.img, p.ldi, 1, item0, p.V, chunks, tid);
        __syncthreads();
        const bool ok0 = item0 + r < p.V, ok1 = item0 + 32 + r < p.V;
        const int c0 = (int)(item0 + r), c1 = (int)(item0 + 32 + r);    // used where ok0 / ok1: V is an int, so are they
        for (int rb = wave * 32; rb < p.n_rows; rb += 128) {    // wave-uniform
            const uint4* ap = reinterpret_cast<const uint4*>(p.x16 + (long)min(rb + r, p.n_rows - 1) * p.ldp) + h;
            f32x16 acc[2];
            itk16_product<DT>(ap, b0p, b1p, nk, acc);
            float km = ninf, ks = 0.f, kq = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = rb + itk16_acc_row(e, h), rc = min(row, p.n_rows - 1);
                const float tg = p.target[rc];
                const int lab = (int)p.labels[rc];          // a label outside [0, V) has a NaN target: no hit whatever this is
                const float v0 = alpha * acc[0][e], v1 = alpha * acc[1][e];
                const unsigned long long m0 = __ballot(ok0 && (v0 > tg || (v0 == tg && c0 < lab)));
                const unsigned long long m1 = __ballot(ok1 && (v1 > tg || (v1 == tg && c1 < lab)));
                const int cnt = h ? __popc((unsigned)(m0 >> 32)) + __popc((unsigned)(m1 >> 32))
                                  : __popc((unsigned)m0) + __popc((unsigned)m1);
                if (r == 0 && cnt && row < p.n_rows) atomicAdd(p.rank + row, cnt);
                const float w0 = ok0 ? v0 : ninf, w1 = ok1 ? v1 : ninf;
                const float bm = row16_max(fmaxf(w0, w1));
                const float sh = bm == ninf ? 0.f : bm;
                const float bs = row16_sum(__expf(w0 - sh) + __expf(w1 - sh));
                const float bq = row16_sum((ok0 ? v0 : 0.f) + (ok1 ? v1 : 0.f));
                if ((r & 15) == e) { km = bm; ks = bs; kq = bq; }
            }
            // the other 16-lane row of the half holds the rest of the same block row
            lse_merge(km, ks, __shfl_xor(km, 16, 64), __shfl_xor(ks, 16, 64));
            kq += __shfl_xor(kq, 16, 64);
            if (r < 16 && rb + krow < p.n_rows) {
                float4 st = make_float4(ninf, 0.f, 0.f, 0.f);
                if (t > t0) st = part[rb + krow];
                lse_merge(st.x, st.y, km, ks);
                st.z += kq;
                part[rb + krow] = st;
            }
        }
    }
}

// 4 rows x 64 chains per workgroup: chain c of a row folds groups c, c + 64, ... in order, then the 64 chains merge pairwise
__global__ __launch_bounds__(256) void itev16_finalise_kernel(Itev16Params p) {
    __shared__ float sm[64][4], ss[64][4], sq[64][4];
    const int rr = threadIdx.x & 3, c = threadIdx.x >> 2;
    const int row = blockIdx.x * 4 + rr;
    float m = -__builtin_inff(), s = 0.f, q = 0.f;
    if (row < p.n_rows) {
        for (int g = c; g < p.groups; g += 64) {
            const float4 st = p.part[(long)g * p.n_rows + row];
            lse_merge(m, s, st.x, st.y);
            q += st.z;
        }
    }
    sm[c][rr] = m; ss[c][rr] = s; sq[c][rr] = q;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) {
        if (c < o) {
            lse_merge(m, s, sm[c + o][rr], ss[c + o][rr]);
            q += sq[c + o][rr];
            sm[c][rr] = m; ss[c][rr] = s; sq[c][rr] = q;
        }
        __syncthreads();
    }
    if (c == 0 && row < p.n_rows) {
        p.lse[row] = m + logf(s);
        p.score_sum[row] = q;
    }
}

T4rLdsAttr g_lds_attr[2];

template <int DT>
int launch_t(hipStream_t st, const Itev16Params& p) {
    hipLaunchKernelGGL((itev16_target_kernel<DT>), dim3((unsigned)((p.n_rows + 31) / 32)), dim3(64), 0, st, p);
    T4R_LAUNCH_CHECK();
    const size_t smem = itk16_lds_bytes(p.ldp);
    t4r_ensure_dynamic_lds((const void*)itev16_kernel<DT>, smem, g_lds_attr[DT - 2]);
    hipLaunchKernelGGL((itev16_kernel<DT>), dim3((unsigned)p.groups), dim3(256), smem, st, p);
    T4R_LAUNCH_CHECK();
    hipLaunchKernelGGL(itev16_finalise_kernel, dim3((unsigned)((p.n_rows + 3) / 4)), dim3(256), 0, st, p);
    T4R_LAUNCH_CHECK();
    return 0;
}

// the split of V over workgroups: from V alone
void split_of(long V, int& G, long& tiles, int& groups) {
    tiles = (V + ITK16_TILE - 1) / ITK16_TILE;
    long g = (tiles + ITEV16_GROUPS - 1) / ITEV16_GROUPS;
    g = g < 1 ? 1 : (g > ITEV16_MAX_G ? ITEV16_MAX_G : g);
    G = (int)g;
    groups = (int)((tiles + g - 1) / g);
}

size_t x16_bytes(long n_rows, long kp) { return ((size_t)n_rows * kp * 2 + 255) & ~(size_t)255; }

}  // namespace

extern "C" long t4r_item_eval_h16_ws_bytes(int n_rows, int V, int D) {
    if (n_rows <= 0 || V <= 0 || D <= 0) return 0;
    // sized for the most groups any V' <= V can have (the count itself steps down where G steps up): never decreases in V
    const long tiles = ((long)V + ITK16_TILE - 1) / ITK16_TILE;
    const long most = tiles <= ITEV16_GROUPS ? tiles : std::max((long)ITEV16_GROUPS, (tiles + ITEV16_MAX_G - 1) / ITEV16_MAX_G);
    return (long)(x16_bytes(n_rows, itk16_image_ld(D)) + (size_t)most * n_rows * sizeof(float4));
}

extern "C" int t4r_item_eval_h16(void* stream, int n_rows, int V, int D, float alpha, const float* X, long ldx, const void* image,
                                 long ldp, int dtype, const long* labels, float* lse, float* target, float* score_sum, int* rank,
                                 void* workspace, long ws_bytes) {
    if (n_rows == 0) return 0;
    T4R_CHECK_ARG(n_rows > 0 && V > 0 && D > 0 && X && image, "item_eval_h16: bad arguments");
    T4R_CHECK_ARG(labels && lse && target && score_sum && rank, "item_eval_h16: labels and the four outputs must not be null");
    T4R_CHECK_ARG(itk16_supported(D), "item_eval_h16: 1 <= D <= 512 (t4r_item_topk_h16_supported)");
    T4R_CHECK_ARG(ldx >= D, "item_eval_h16: row pitch below D");
    ITK16_CHECK_IMAGE("item_eval_h16");
    const long kp = itk16_image_ld(D);
    T4R_CHECK_ARG(workspace && ws_bytes >= t4r_item_eval_h16_ws_bytes(n_rows, V, D) && (uintptr_t)workspace % 16 == 0,
                  "item_eval_h16: workspace too small (t4r_item_eval_h16_ws_bytes) or not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    uint16_t* x16 = (uint16_t*)workspace;
    int rc = t4r_itk16_round_rows(st, dtype, X, ldx, n_rows, D, x16, kp);
    if (rc) return rc;
    Itev16Params p = {};
    p.n_rows = n_rows; p.V = V; p.ldp = (int)kp; p.x16 = x16; p.img = (const uint16_t*)image; p.ldi = ldp; p.alpha = alpha;
    p.labels = labels; p.target = target; p.rank = rank; p.lse = lse; p.score_sum = score_sum;
    p.part = (float4*)((char*)workspace + x16_bytes(n_rows, kp));
    split_of(V, p.G, p.tiles, p.groups);
    return itk16_dispatch(dtype, [&](auto dt) { return launch_t<decltype(dt)::value>(st, p); });
}
