// GRU body (include/t4r_hip_gru.h): a stack of 1 .. 4 GRU layers over [B, L, K0], and the backward of all of it.  gfx950 only.
//
// Recurrence, one launch per layer for the whole time loop.  A workgroup owns 16 consecutive sessions and has HT / 16 waves
// (HT = H rounded up to 32, 64 or 128).  Wave w owns the hidden units 16 w .. 16 w + 15 of all three gates: its rows of W_hh
// stay in REGISTERS for all L steps as the A operand of v_mfma_f32_16x16x4_f32 (lane (c, q) = (lane & 15, lane >> 4) supplies
// A[unit 16 w + c][k = 4 s + q] in step s: 3 HT / 4 registers, 96 at H = 128 over eight waves), so nothing of W_hh is read
// again after the prologue.  The B operand is h_{t-1} of the 16 sessions, [k][session] with pitch 16 in LDS: the read of rows
// 4 s + q is one conflict-free run of 64 floats.  The accumulator image -- lane (c, q) holds units 16 w + 4 q + r, r < 4, of
// session c -- has r, z and n of one (unit, session) in one lane, so the gate arithmetic needs no exchange; the new h goes to the
// OTHER of two LDS buffers, and ONE barrier per step orders it before the next step's reads (a wave can be at most one step
// ahead, and then writes the buffer nobody reads).  A tail tile computes on the last session and masks its stores; padded units
// (>= H) have zero weights and stay exactly 0.  Every wave reaches every barrier.
// The time-reversed recurrence has the same form with W_hh^T in registers (wave w owns the units 16 w .. of the carry, the
// contraction runs over the 3 HT gate rows: again 3 HT / 4 registers) and dgh of the step exchanged through LDS.
// The products around it (gi = b_ih + a W_ih^T for all tokens, d a = dgi W_ih, the [d W | d b] partials and their sums) are the
// forms of mlp_block.hip: one wave per 32 tokens on v_mfma_f32_32x32x2_f32, k ascending; the weight gradients one wave per
// 64 x 64 tile and split of the token range, partials added in split order.  No float atomics.
#include "../../include/t4r_hip_gru.h"
#include "mfma_frag.h"
#include <limits.h>

#define GR_MAX_LAYERS 4
#define GR_MAX_K0 1024
#define GR_MAX_H 128
#define GR_MAX_L 1023
#define GR_SITE 9                      // T4R_SITE_GRU: the dropout site of this block (layer byte = the layer's index)
#define GR_PART_FLOATS (8l << 20)      // [d W | d b] partials of one layer: at most 8 Mi floats
#define GR_MAX_SPLITS 1024
#define GR_MAX_BLOCKS (1l << 20)       // grid-stride kernels
#define GR_TILE 16                     // sessions per workgroup of the recurrence kernels

typedef float f32x4 __attribute__((ext_vector_type(4)));

extern "C" unsigned long long t4r_dropout_ctr_hi(unsigned long long offset, int layer, int site);

static inline bool gr_dims_ok(int n, int K0, int H, int L) {
    return n >= 1 && n <= GR_MAX_LAYERS && K0 >= 1 && K0 <= GR_MAX_K0 && H >= 1 && H <= GR_MAX_H && L >= 1 && L <= GR_MAX_L;
}
static inline bool gr_batch_ok(long B, int L, int K0, int H) {
    const long wmax = K0 > 3 * H ? K0 : 3 * H;
    return B >= 0 && B <= INT_MAX && B * L * wmax <= INT_MAX;
}
static inline long gr_round4(long v) { return (v + 3) & ~3l; }
// floats of one split's partials of one layer: [3H, K + 1] and [3H, H + 1], K the widest input
static inline long gr_part_floats(int K0, int H) { return 3l * H * ((K0 > H ? K0 : H) + 1) + 3l * H * (H + 1); }
static inline long gr_splits(long T, long part) {
    long s = (T + 63) / 64, cap = GR_PART_FLOATS / part;                      // cap >= 18 within the limits
    if (cap > GR_MAX_SPLITS) cap = GR_MAX_SPLITS;
    return s < cap ? s : cap;
}

extern "C" int t4r_gru_supported(int n, int K0, int H, int L) { return gr_dims_ok(n, K0, H, L) ? 1 : 0; }

extern "C" long t4r_gru_saved_floats(long B, int L, int n, int K0, int H) {
    if (!gr_dims_ok(n, K0, H, L) || B <= 0 || !gr_batch_ok(B, L, K0, H)) return 0;
    return B * L * H * (6l * (n - 1) + 4);
}
extern "C" long t4r_gru_fwd_ws_floats(long B, int L, int n, int K0, int H) {
    if (!gr_dims_ok(n, K0, H, L) || B <= 0 || !gr_batch_ok(B, L, K0, H)) return 0;
    return gr_round4(B * L * 3 * H) + (long)(n - 1) * gr_round4(B * L * H);
}
extern "C" long t4r_gru_bwd_ws_floats(long B, int L, int n, int K0, int H) {
    if (!gr_dims_ok(n, K0, H, L) || B <= 0 || !gr_batch_ok(B, L, K0, H)) return 0;
    const long T = B * L, part = gr_part_floats(K0, H);
    return gr_round4(T * 3 * H) + 2 * gr_round4(T * H) + gr_splits(T, part) * part;
}

namespace {

// ---- the recurrence kernels ------------------------------------------------------------------------------------------------
struct GRRec {
    const float* gi;        // fwd: [T, 3H]
    const float* Whh;       // [3H, H]
    const float* bhh;       // fwd: [3H] or null
    const float* h0;        // [B, H] of this layer, or null
    float* hout;            // fwd: where the undropped h is stored, or null;  bwd: read (h of this layer, [T, H])
    float* yout;            // fwd: where h * mask is stored (the next layer's input), or null
    float* gates;           // fwd: where r | z | n | gh_n [T, 4H] are stored, or null;  bwd: read
    const float* dout;      // bwd: [T, H]
    float* dgi;             // bwd: [T, 3H]
    float* dghn;            // bwd: [T, H]
    long B;
    int L, H, vec, mask_dout;
    DropCfg drop;           // fwd: the mask of yout;  bwd: the mask of dout (the layer's own output mask) where mask_dout
};

__device__ __forceinline__ float gr_sig(float v) { return 1.f / (1.f + expf(-v)); }
__device__ __forceinline__ float gr_tanh(float v) { return 1.f - 2.f / (1.f + expf(2.f * v)); }

// p[d .. d + 3] of a row whose units below H exist
__device__ __forceinline__ f32x4 gr_ld4(const float* p, int d, int H, bool vec) {
    f32x4 v;
    if (vec) {
        const float4 t = *reinterpret_cast<const float4*>(p + d);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        return v;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = d + r < H ? p[d + r] : 0.f;
    return v;
}
__device__ __forceinline__ void gr_st4(float* p, int d, int H, bool vec, const f32x4 v) {
    if (vec) { *reinterpret_cast<float4*>(p + d) = make_float4(v[0], v[1], v[2], v[3]); return; }
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (d + r < H) p[d + r] = v[r];
}
// the dropout factors of units d .. d + 3 of token row tok of a [T, H] site
__device__ __forceinline__ f32x4 gr_drop4(const DropCfg& dc, long tok, int d, int H) {
    const unsigned long long idx = (unsigned long long)tok * (unsigned long long)H + (unsigned long long)d;
    f32x4 m;
    if ((H & 3) == 0) {                                      // d % 4 == 0: the four elements are one Philox block
        const float4 t = drop_scale4(dc, idx);
        m[0] = t.x; m[1] = t.y; m[2] = t.z; m[3] = t.w;
        return m;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) m[r] = d + r < H ? drop_scale(dc, idx + r) : 0.f;
    return m;
}

template <int HT>
__global__ __launch_bounds__(HT * 4) void gr_fwd_kernel(GRRec a) {
    constexpr int KS = HT / 4;
    __shared__ float hs[2][HT * GR_TILE];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    const int H = a.H, L = a.L;
    const long sb = (long)blockIdx.x * GR_TILE + c;
    const bool live = sb < a.B;
    const long sc = live ? sb : a.B - 1;                     // a tail tile computes on the last session and stores nothing
    const int d0 = 16 * w + 4 * q;                           // the lane's units d0 .. d0 + 3 of session c
    const bool vec = a.vec != 0;
    const bool any = d0 < H;
    float wr[KS], wz[KS], wn[KS];
    {
        const int row = 16 * w + c;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int k = 4 * s + q;
            const bool ok = row < H && k < H;
            const long o = ok ? (long)row * H + k : 0;
            wr[s] = ok ? a.Whh[o] : 0.f;
            wz[s] = ok ? a.Whh[(long)H * H + o] : 0.f;
            wn[s] = ok ? a.Whh[2l * H * H + o] : 0.f;
        }
    }
    f32x4 br, bz, bn, hp;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const bool ok = d0 + r < H;
        br[r] = ok && a.bhh ? a.bhh[d0 + r] : 0.f;
        bz[r] = ok && a.bhh ? a.bhh[H + d0 + r] : 0.f;
        bn[r] = ok && a.bhh ? a.bhh[2 * H + d0 + r] : 0.f;
        hp[r] = ok && a.h0 ? a.h0[sc * H + d0 + r] : 0.f;
        hs[0][(d0 + r) * GR_TILE + c] = hp[r];
    }
    __syncthreads();
    const bool dropping = a.drop.p > 0.f;
    for (int t = 0; t < L; ++t) {
        const long tok = sc * L + t;
        const float* girow = a.gi + tok * 3 * H;
        f32x4 gr = {0.f, 0.f, 0.f, 0.f}, gz = gr, gn = gr;
        if (any) { gr = gr_ld4(girow, d0, H, vec); gz = gr_ld4(girow + H, d0, H, vec); gn = gr_ld4(girow + 2 * H, d0, H, vec); }
        f32x4 ar = br, az = bz, an = bn;
        const float* hb = hs[t & 1];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const float hv = hb[(4 * s + q) * GR_TILE + c];
            ar = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[s], hv, ar, 0, 0, 0);
            az = __builtin_amdgcn_mfma_f32_16x16x4f32(wz[s], hv, az, 0, 0, 0);
            an = __builtin_amdgcn_mfma_f32_16x16x4f32(wn[s], hv, an, 0, 0, 0);
        }
        f32x4 rr, zz, nn, hn;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            rr[r] = gr_sig(gr[r] + ar[r]);
            zz[r] = gr_sig(gz[r] + az[r]);
            nn[r] = gr_tanh(gn[r] + rr[r] * an[r]);
            hn[r] = nn[r] + zz[r] * (hp[r] - nn[r]);
        }
        float* hnext = hs[(t + 1) & 1];
#pragma unroll
        for (int r = 0; r < 4; ++r) hnext[(d0 + r) * GR_TILE + c] = hn[r];
        if (live && any) {
            if (a.hout) gr_st4(a.hout + tok * H, d0, H, vec, hn);
            if (a.yout) {
                f32x4 y = hn;
                if (dropping) {
                    const f32x4 m = gr_drop4(a.drop, tok, d0, H);
#pragma unroll
                    for (int r = 0; r < 4; ++r) y[r] = __fmul_rn(hn[r], m[r]);
                }
                gr_st4(a.yout + tok * H, d0, H, vec, y);
            }
            if (a.gates) {
                float* g = a.gates + tok * 4 * H;
                gr_st4(g, d0, H, vec, rr); gr_st4(g + H, d0, H, vec, zz); gr_st4(g + 2 * H, d0, H, vec, nn);
                gr_st4(g + 3 * H, d0, H, vec, an);
            }
        }
        hp = hn;
        __syncthreads();
    }
}

template <int HT>
__global__ __launch_bounds__(HT * 4) void gr_bwd_kernel(GRRec a) {
    constexpr int KS = 3 * HT / 4;
    __shared__ float gs[2][3 * HT * GR_TILE];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    const int H = a.H, L = a.L;
    const long sb = (long)blockIdx.x * GR_TILE + c;
    const bool live = sb < a.B;
    const long sc = live ? sb : a.B - 1;
    const int d0 = 16 * w + 4 * q;
    const bool vec = a.vec != 0;
    const bool any = d0 < H;
    float wt[KS];                                            // W_hh[gate row 4 s + q of the padded [3][HT] order][unit 16 w + c]
    {
        const int col = 16 * w + c;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int ii = 4 * s + q, g = ii / HT, dd = ii % HT;
            const bool ok = dd < H && col < H;
            wt[s] = ok ? a.Whh[((long)g * H + dd) * H + col] : 0.f;
        }
    }
    f32x4 carry = {0.f, 0.f, 0.f, 0.f};
    const f32x4 zero = carry;
    for (int t = L - 1; t >= 0; --t) {
        const long tok = sc * L + t;
        f32x4 dy = zero, rr = zero, zz = zero, nn = zero, gh = zero, hp = zero;
        if (any) {
            dy = gr_ld4(a.dout + tok * H, d0, H, vec);
            if (a.mask_dout) {
                const f32x4 m = gr_drop4(a.drop, tok, d0, H);
#pragma unroll
                for (int r = 0; r < 4; ++r) dy[r] = __fmul_rn(dy[r], m[r]);
            }
            const float* g = a.gates + tok * 4 * H;
            rr = gr_ld4(g, d0, H, vec); zz = gr_ld4(g + H, d0, H, vec); nn = gr_ld4(g + 2 * H, d0, H, vec);
            gh = gr_ld4(g + 3 * H, d0, H, vec);
            if (t > 0) hp = gr_ld4(a.hout + (tok - 1) * H, d0, H, vec);
            else if (a.h0) hp = gr_ld4(a.h0 + sc * H, d0, H, vec);
        }
        f32x4 dpr, dpz, dpn, dgn, acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float dh = dy[r] + carry[r];
            dpn[r] = dh * (1.f - zz[r]) * (1.f - nn[r] * nn[r]);
            dpz[r] = dh * (hp[r] - nn[r]) * (zz[r] * (1.f - zz[r]));
            dpr[r] = dpn[r] * gh[r] * (rr[r] * (1.f - rr[r]));
            dgn[r] = dpn[r] * rr[r];
            acc[r] = dh * zz[r];
        }
        float* gb = gs[t & 1];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            gb[(d0 + r) * GR_TILE + c] = dpr[r];
            gb[(HT + d0 + r) * GR_TILE + c] = dpz[r];
            gb[(2 * HT + d0 + r) * GR_TILE + c] = dgn[r];
        }
        if (live && any) {
            float* o = a.dgi + tok * 3 * H;
            gr_st4(o, d0, H, vec, dpr); gr_st4(o + H, d0, H, vec, dpz); gr_st4(o + 2 * H, d0, H, vec, dpn);
            gr_st4(a.dghn + tok * H, d0, H, vec, dgn);
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[s], gb[(4 * s + q) * GR_TILE + c], acc, 0, 0, 0);
        carry = acc;
    }
}

// ---- the token-wise products -------------------------------------------------------------------------------------------------
struct GRLin {
    const float* a;         // [T, K]   (gi: the layer's input;  dx: dgi [T, N])
    const float* W;         // [N, K]
    const float* bias;      // gi: [N] or null
    float* out;             // gi: [T, N];  dx: [T, K]
    long T;
    int K, N, vin, vout;
};

__device__ __forceinline__ float4 gr_row_ld4(const float* p, int k, int n, bool vec) {
    if (vec) return *reinterpret_cast<const float4*>(p + k);
    float4 v;
    v.x = k < n ? p[k] : 0.f;
    v.y = k + 1 < n ? p[k + 1] : 0.f;
    v.z = k + 2 < n ? p[k + 2] : 0.f;
    v.w = k + 3 < n ? p[k + 3] : 0.f;
    return v;
}
__device__ __forceinline__ void gr_row_st4(float* p, int k, int n, bool vec, const float4 v) {
    if (vec) { *reinterpret_cast<float4*>(p + k) = v; return; }
    if (k < n) p[k] = v.x;
    if (k + 1 < n) p[k + 1] = v.y;
    if (k + 2 < n) p[k + 2] = v.z;
    if (k + 3 < n) p[k + 3] = v.w;
}

// out[t][d] = bias[d] + sum_k a[t][k] W[d][k], k ascending; one wave per 32 tokens and 128 output columns (blockIdx.y)
__global__ __launch_bounds__(64) void gr_gi_kernel(GRLin a) {
    const int lane = threadIdx.x, c = lane & 31, kh = lane >> 5;
    const long t = (long)blockIdx.x * 32 + c;
    const bool live = t < a.T;
    const long tc = live ? t : a.T - 1;
    const int K = a.K, N = a.N, d0 = blockIdx.y * 128;
    const bool vin = a.vin != 0, vout = a.vout != 0;
    const float* xrow = a.a + tc * K;
    f32x16 acc[4];
    const float* wrow[4];
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
        const int dw = d0 + 32 * qq + c;
        wrow[qq] = a.W + (long)(dw < N ? dw : N - 1) * K;                     // rows past N compute on row N - 1, never stored
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int d = d0 + 32 * qq + xm_row(r, kh);
            acc[qq][r] = a.bias ? a.bias[d < N ? d : N - 1] : 0.f;
        }
    }
    for (int k = 0; k < K; k += 4) {
        const float4 xv = gr_row_ld4(xrow, k, K, vin);
        const float x0 = kh ? xv.y : xv.x, x1 = kh ? xv.w : xv.z;
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            if (d0 + 32 * qq >= N) continue;                                   // wave uniform
            const float4 wv = gr_row_ld4(wrow[qq], k, K, vin);
            acc[qq] = __builtin_amdgcn_mfma_f32_32x32x2f32(kh ? wv.y : wv.x, x0, acc[qq], 0, 0, 0);
            if (k + 2 < K) acc[qq] = __builtin_amdgcn_mfma_f32_32x32x2f32(kh ? wv.w : wv.z, x1, acc[qq], 0, 0, 0);
        }
    }
    if (!live) return;
    float* orow = a.out + tc * N;
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d = d0 + 32 * qq + 8 * g + 4 * kh;
            if (d >= N) continue;
            gr_row_st4(orow, d, N, vout, make_float4(acc[qq][4 * g], acc[qq][4 * g + 1], acc[qq][4 * g + 2], acc[qq][4 * g + 3]));
        }
    }
}

// out[t][k] = sum_d a[t][d] W[d][k], d ascending; one wave per 32 tokens and 128 columns k (blockIdx.y)
__global__ __launch_bounds__(64) void gr_dx_kernel(GRLin a) {
    const int lane = threadIdx.x, c = lane & 31, kh = lane >> 5;
    const long t = (long)blockIdx.x * 32 + c;
    const bool live = t < a.T;
    const long tc = live ? t : a.T - 1;
    const int K = a.K, N = a.N, k0 = blockIdx.y * 128;
    const float* grow = a.a + tc * N;
    f32x16 acc[4];
    int col[4];
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
        acc[qq] = zero16();
        const int kc = k0 + 32 * qq + c;
        col[qq] = kc < K ? kc : K - 1;                                         // columns past K compute on column K - 1, never stored
    }
    for (int d = 0; d < N; d += 2) {
        const bool ok = d + kh < N;                                            // N odd: the last step's second slot is fma(0, 0, acc)
        const float g = ok ? grow[d + kh] : 0.f;
        const float* wr = a.W + (long)(ok ? d + kh : N - 1) * K;
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            if (k0 + 32 * qq >= K) continue;                                   // wave uniform
            const float wv = ok ? wr[col[qq]] : 0.f;
            acc[qq] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, g, acc[qq], 0, 0, 0);
        }
    }
    if (!live) return;
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int k = k0 + 32 * qq + 8 * g + 4 * kh;
            if (k >= K) continue;
            gr_row_st4(a.out + tc * K, k, K, a.vout != 0,
                       make_float4(acc[qq][4 * g], acc[qq][4 * g + 1], acc[qq][4 * g + 2], acc[qq][4 * g + 3]));
        }
    }
}

// ---- the weight gradients ----------------------------------------------------------------------------------------------------
// job 0: [d W_ih | d b_ih] = sum_tok dgi^T [a | 1];  job 1: [d W_hh | d b_hh] = sum_tok dgh^T [h_{t-1} | 1], dgh = dgi with its n
// part taken from dghn, h_{t-1} the row above in hout or, at t = 0, the session's row of h0 (null: zeros)
struct GRDw {
    const float* dgi;       // [T, 3H]
    const float* dghn;      // [T, H]
    const float* ain;       // [T, K]: the layer's input
    const float* hout;      // [T, H]: the layer's h
    const float* h0;        // [B, H] or null
    float* part;            // [job: part_off][splits][3H][C + 1]
    float* dW[2]; float* db[2];
    long part_off[2];
    long T;
    int L, H, K, tiles0, splits, kper;   // tiles0: 64 x 64 tiles of job 0 (0 where it is not wanted)
    int want[2];
};

__global__ __launch_bounds__(64) void gr_dw_kernel(GRDw a) {
    const int job = (int)blockIdx.x >= a.tiles0 ? 1 : 0;
    const int tile = (int)blockIdx.x - (job ? a.tiles0 : 0);
    const int H = a.H, D = 3 * H, C = job ? H : a.K, C1 = C + 1, lane = threadIdx.x, c = lane & 31, kh = lane >> 5;
    const int tilesC = (C1 + 63) >> 6;
    const int dI = (tile / tilesC) << 6, cJ = (tile % tilesC) << 6;
    const long k0 = (long)blockIdx.y * a.kper;
    const long k1 = k0 + a.kper < a.T ? k0 + a.kper : a.T;
    const bool d1 = dI + 32 < D, c1 = cJ + 32 < C1;                   // wave uniform: the second half of the tile exists
    const int da = min(dI + c, D - 1), db = min(dI + 32 + c, D - 1);
    const int ca = cJ + c, cb = cJ + 32 + c;                          // >= C: the ones column (past it: never stored)
    f32x16 o00 = zero16(), o01 = zero16(), o10 = zero16(), o11 = zero16();
    auto gsrc = [&](long tr, int d) -> float {
        return job && d >= 2 * H ? a.dghn[tr * H + (d - 2 * H)] : a.dgi[tr * D + d];
    };
    auto psrc = [&](long tr, int col) -> float {
        if (col >= C) return 1.f;
        if (!job) return a.ain[tr * C + col];
        const long b = tr / a.L;
        if (tr - b * a.L > 0) return a.hout[(tr - 1) * H + col];
        return a.h0 ? a.h0[b * H + col] : 0.f;
    };
    for (long tt = k0; tt < k1; tt += 2) {
        const long tk = tt + kh;
        const bool okt = tk < k1;
        const long tr = okt ? tk : k1 - 1;                            // every load is in bounds; a token past the split counts 0
        const float a0 = okt ? gsrc(tr, da) : 0.f, a1 = okt ? gsrc(tr, db) : 0.f;
        const float b0 = psrc(tr, ca), b1 = psrc(tr, min(cb, C));
        o00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, o00, 0, 0, 0);
        if (c1) o01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, o01, 0, 0, 0);
        if (d1) o10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, o10, 0, 0, 0);
        if (d1 && c1) o11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, o11, 0, 0, 0);
    }
    float* out = a.part + a.part_off[job] + (long)blockIdx.y * D * C1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int d = dI + xm_row(r, kh);
        if (d < D && ca < C1) out[(long)d * C1 + ca] = o00[r];
        if (d < D && cb < C1) out[(long)d * C1 + cb] = o01[r];
        if (d + 32 < D && ca < C1) out[(long)(d + 32) * C1 + ca] = o10[r];
        if (d + 32 < D && cb < C1) out[(long)(d + 32) * C1 + cb] = o11[r];
    }
}

// element e of a job's [d W | d b]: its partials in split order, then one add into the caller's gradient
__global__ __launch_bounds__(256) void gr_finish_kernel(GRDw a, long n0, long total) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int job = i >= n0 ? 1 : 0;
        if (!a.want[job]) continue;
        const long e = job ? i - n0 : i;
        const int C = job ? a.H : a.K, C1 = C + 1;
        const long nW = 3l * a.H * C1;
        const int d = (int)(e / C1), cc = (int)(e - (long)d * C1);
        float* dst = cc < C ? (a.dW[job] ? a.dW[job] + (long)d * C + cc : nullptr) : (a.db[job] ? a.db[job] + d : nullptr);
        if (!dst) continue;
        const float* p = a.part + a.part_off[job];
        float s = p[e];
#pragma unroll 8
        for (int k = 1; k < a.splits; ++k) s += p[(long)k * nW + e];
        *dst += s;
    }
}

template <int HT>
static void gr_launch_fwd(const GRRec& a, hipStream_t st) {
    hipLaunchKernelGGL(gr_fwd_kernel<HT>, dim3((unsigned)((a.B + GR_TILE - 1) / GR_TILE)), dim3(HT * 4), 0, st, a);
}
template <int HT>
static void gr_launch_bwd(const GRRec& a, hipStream_t st) {
    hipLaunchKernelGGL(gr_bwd_kernel<HT>, dim3((unsigned)((a.B + GR_TILE - 1) / GR_TILE)), dim3(HT * 4), 0, st, a);
}

}  // namespace

#define GR_A4(p) ((uintptr_t)(p) % 4 == 0)
#define GR_A16(p) ((uintptr_t)(p) % 16 == 0)
// the sizes both directions share: checked first, and nothing is dereferenced
#define GR_CHECK_DIMS(name)                                                                                  \
    T4R_CHECK_ARG(n >= 1 && n <= GR_MAX_LAYERS, name ": 1 <= n <= 4 layers");                                \
    T4R_CHECK_ARG(K0 >= 1 && K0 <= GR_MAX_K0, name ": 1 <= K0 <= 1024");                                     \
    T4R_CHECK_ARG(H >= 1 && H <= GR_MAX_H, name ": 1 <= H <= 128");                                          \
    T4R_CHECK_ARG(L >= 1 && L <= GR_MAX_L, name ": 1 <= L <= 1023");                                         \
    T4R_CHECK_ARG(gr_batch_ok(B, L, K0, H), name ": B >= 0 and B L max(K0, 3H) < 2^31");                     \
    T4R_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, name ": 0 <= drop_p < 1");                                  \
    if (B == 0) return 0

extern "C" int t4r_gru_fwd(void* stream, const float* x, const float* h0, const float* const* W_ih, const float* const* W_hh,
                           const float* const* b_ih, const float* const* b_hh, float* out, float* saved, float* ws, long B, int L,
                           int n, int K0, int H, float drop_p, unsigned long long seed, unsigned long long offset) {
    GR_CHECK_DIMS("gru_fwd");
    T4R_CHECK_ARG(x && W_ih && W_hh && out && ws, "gru_fwd: null pointer (x, W_ih, W_hh, out or ws)");
    T4R_CHECK_ARG(GR_A4(x) && GR_A4(h0) && GR_A4(out) && GR_A4(saved) && GR_A4(ws), "gru_fwd: every pointer must be 4-byte aligned");
    for (int k = 0; k < n; ++k) {
        T4R_CHECK_ARG(W_ih[k] && W_hh[k], "gru_fwd: null pointer (W_ih[k] or W_hh[k])");
        T4R_CHECK_ARG(GR_A4(W_ih[k]) && GR_A4(W_hh[k]) && (!b_ih || GR_A4(b_ih[k])) && (!b_hh || GR_A4(b_hh[k])),
                      "gru_fwd: every pointer must be 4-byte aligned");
    }
    const long T = B * L, TH = T * H;
    float* gi = ws;
    float* ybuf = ws + gr_round4(T * 3 * H);
    hipStream_t st = (hipStream_t)stream;
    const float* ain = x;
    for (int k = 0; k < n; ++k) {
        const int K = k ? H : K0;
        const bool last = k == n - 1;
        GRLin g = {};
        g.a = ain; g.W = W_ih[k]; g.bias = b_ih ? b_ih[k] : nullptr; g.out = gi; g.T = T; g.K = K; g.N = 3 * H;
        g.vin = K % 4 == 0 && GR_A16(ain) && GR_A16(g.W);
        g.vout = (3 * H) % 4 == 0 && GR_A16(gi);
        hipLaunchKernelGGL(gr_gi_kernel, dim3((unsigned)((T + 31) / 32), (unsigned)((3 * H + 127) / 128)), dim3(64), 0, st, g);
        T4R_LAUNCH_CHECK();
        GRRec a = {};
        a.gi = gi; a.Whh = W_hh[k]; a.bhh = b_hh ? b_hh[k] : nullptr; a.h0 = h0 ? h0 + (long)k * B * H : nullptr;
        a.B = B; a.L = L; a.H = H;
        a.drop = make_drop(last ? 0.f : drop_p, seed, t4r_dropout_ctr_hi(offset, k, GR_SITE));
        if (saved) {
            float* base = saved + (long)k * 6 * TH;
            a.gates = base;
            a.hout = last ? out : base + 4 * TH;
            a.yout = !last && drop_p > 0.f ? base + 5 * TH : nullptr;
            ain = a.yout ? a.yout : a.hout;
        } else {
            a.hout = last ? out : nullptr;
            a.yout = last ? nullptr : ybuf + (long)k * gr_round4(TH);
            ain = a.yout;
        }
        a.vec = H % 4 == 0 && GR_A16(gi) && GR_A16(a.hout) && GR_A16(a.yout) && GR_A16(a.gates) && GR_A16(a.h0);
        if (H <= 32) gr_launch_fwd<32>(a, st);
        else if (H <= 64) gr_launch_fwd<64>(a, st);
        else gr_launch_fwd<128>(a, st);
        T4R_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int t4r_gru_bwd(void* stream, const float* dout, const float* x, const float* h0, const float* const* W_ih,
                           const float* const* W_hh, const float* out, const float* saved, float* dx, float* const* d_W_ih,
                           float* const* d_W_hh, float* const* d_b_ih, float* const* d_b_hh, float* ws, long B, int L, int n, int K0,
                           int H, float drop_p, unsigned long long seed, unsigned long long offset) {
    GR_CHECK_DIMS("gru_bwd");
    T4R_CHECK_ARG(dout && W_ih && W_hh && out && saved && ws, "gru_bwd: null pointer (dout, W_ih, W_hh, out, saved or ws)");
    T4R_CHECK_ARG(GR_A4(dout) && GR_A4(x) && GR_A4(h0) && GR_A4(out) && GR_A4(saved) && GR_A4(dx) && GR_A4(ws),
                  "gru_bwd: every pointer must be 4-byte aligned");
    bool want[GR_MAX_LAYERS], any_w = false;
    for (int k = 0; k < n; ++k) {
        T4R_CHECK_ARG(W_ih[k] && W_hh[k], "gru_bwd: null pointer (W_ih[k] or W_hh[k])");
        float* g[4] = {d_W_ih ? d_W_ih[k] : nullptr, d_W_hh ? d_W_hh[k] : nullptr, d_b_ih ? d_b_ih[k] : nullptr,
                       d_b_hh ? d_b_hh[k] : nullptr};
        T4R_CHECK_ARG(GR_A4(W_ih[k]) && GR_A4(W_hh[k]) && GR_A4(g[0]) && GR_A4(g[1]) && GR_A4(g[2]) && GR_A4(g[3]),
                      "gru_bwd: every pointer must be 4-byte aligned");
        want[k] = g[0] || g[1] || g[2] || g[3];
        any_w = any_w || want[k];
    }
    T4R_CHECK_ARG(x || !((d_W_ih && d_W_ih[0]) || (d_b_ih && d_b_ih[0])),
                  "gru_bwd: null pointer (x, read for d_W_ih[0] and d_b_ih[0])");
    if (!dx && !any_w) return 0;
    const long T = B * L, TH = T * H;
    float* dgi = ws;
    float* dghn = dgi + gr_round4(T * 3 * H);
    float* dyb = dghn + gr_round4(TH);
    float* part = dyb + gr_round4(TH);
    const long pf = gr_part_floats(K0, H);
    const int splits = (int)gr_splits(T, pf);
    const long kper = (T + splits - 1) / splits;
    hipStream_t st = (hipStream_t)stream;
    int lowest = 0;                                          // the lowest layer whose recurrence has to run
    if (!dx) while (lowest < n && !want[lowest]) ++lowest;
    for (int k = n - 1; k >= lowest; --k) {
        const int K = k ? H : K0;
        const bool last = k == n - 1;
        const float* base = saved + (long)k * 6 * TH;
        const float* hk = last ? out : base + 4 * TH;
        const float* ain = k ? (drop_p > 0.f ? saved + (long)(k - 1) * 6 * TH + 5 * TH : saved + (long)(k - 1) * 6 * TH + 4 * TH) : x;
        const float* h0k = h0 ? h0 + (long)k * B * H : nullptr;
        GRRec a = {};
        a.Whh = W_hh[k]; a.h0 = h0k; a.hout = const_cast<float*>(hk); a.gates = const_cast<float*>(base);
        a.dout = last ? dout : dyb; a.dgi = dgi; a.dghn = dghn; a.B = B; a.L = L; a.H = H;
        a.mask_dout = !last && drop_p > 0.f;
        a.drop = make_drop(last ? 0.f : drop_p, seed, t4r_dropout_ctr_hi(offset, k, GR_SITE));
        a.vec = H % 4 == 0 && GR_A16(a.dout) && GR_A16(hk) && GR_A16(base) && GR_A16(h0k) && GR_A16(dgi) && GR_A16(dghn);
        if (H <= 32) gr_launch_bwd<32>(a, st);
        else if (H <= 64) gr_launch_bwd<64>(a, st);
        else gr_launch_bwd<128>(a, st);
        T4R_LAUNCH_CHECK();
        float* dst = k ? dyb : dx;
        if (k ? k - 1 >= lowest : dx != nullptr) {           // the layer below (or the caller) wants this layer's d input
            GRLin g = {};
            g.a = dgi; g.W = W_ih[k]; g.out = dst; g.T = T; g.K = K; g.N = 3 * H;
            g.vout = K % 4 == 0 && GR_A16(dst);
            hipLaunchKernelGGL(gr_dx_kernel, dim3((unsigned)((T + 31) / 32), (unsigned)((K + 127) / 128)), dim3(64), 0, st, g);
            T4R_LAUNCH_CHECK();
        }
        if (want[k]) {
            GRDw w = {};
            w.dgi = dgi; w.dghn = dghn; w.ain = ain; w.hout = hk; w.h0 = h0k; w.part = part;
            w.dW[0] = d_W_ih ? d_W_ih[k] : nullptr; w.db[0] = d_b_ih ? d_b_ih[k] : nullptr;
            w.dW[1] = d_W_hh ? d_W_hh[k] : nullptr; w.db[1] = d_b_hh ? d_b_hh[k] : nullptr;
            w.want[0] = w.dW[0] || w.db[0]; w.want[1] = w.dW[1] || w.db[1];
            w.T = T; w.L = L; w.H = H; w.K = K; w.splits = splits;
            w.kper = (int)(kper + (kper & 1));
            const long n0 = 3l * H * (K + 1), n1 = 3l * H * (H + 1);
            w.part_off[0] = 0; w.part_off[1] = (long)splits * n0;
            const int rows = (3 * H + 63) / 64;
            w.tiles0 = w.want[0] ? rows * ((K + 1 + 63) / 64) : 0;
            const int tiles = w.tiles0 + (w.want[1] ? rows * ((H + 1 + 63) / 64) : 0);
            hipLaunchKernelGGL(gr_dw_kernel, dim3((unsigned)tiles, (unsigned)splits), dim3(64), 0, st, w);
            T4R_LAUNCH_CHECK();
            const long total = n0 + n1, b = (total + 255) / 256;
            hipLaunchKernelGGL(gr_finish_kernel, dim3((unsigned)(b < GR_MAX_BLOCKS ? b : GR_MAX_BLOCKS)), dim3(256), 0, st, w, n0, total);
            T4R_LAUNCH_CHECK();
        }
    }
    return 0;
}
