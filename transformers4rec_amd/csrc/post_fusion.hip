// Post-context fusion (include/t4r_hip_postfusion.h): out = seq * (1 + p), seq + p or seq | ctx per token, with
// p = b + W ctx the context's projection to the model width, and the backward of all of it.  gfx950 only.
//
// Projected modes (MUL, SUM).  A workgroup of four waves owns 128 consecutive tokens, a wave 32 of them, and walks the model
// width in tiles of 32 rows d.  Per tile the wave forms p^T = W ctx^T on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: bit
// for bit an fp32 fma chain per element, seeded with b[d]) with the token on the lane and d in the 16 registers (mfma_frag.h's
// map).  Step s of the contraction takes c = 2 s + kh, so the chain runs over c ASCENDING: both lane halves read the same four
// consecutive floats of their row of W and of ctx and take elements (0, 2) or (1, 3).  Registers 4 g .. 4 g + 3 are rows
// d0 + 8 g + 4 kh .. + 3: one 16-byte request of seq and of out each.  A token's chain sees only its own row of ctx: the same
// bits alone and in a batch, and in the backward's recomputation (the same function on the same operands).
//   backward, tile kernel: per 32-row tile, dseq = dout (1 + p) (MUL; p recomputed) or dout (SUM), and g = dout seq or dout in
//     the accumulator's register image, which IS the A operand of dctx = g W (the contraction runs over the accumulator's row
//     index d): no exchange.  The dctx accumulators (32 tokens x 32 columns c each, up to eight) stay in registers over the
//     tiles.  A session-level context gets the per-token rows in ws; the finish kernel adds a session's L rows in token order.
//   d W kernel: one wave per 64 x 64 tile of [d_w | d_b] ([D, C + 1]: d_b is the product with a column of ones) and per
//     split of the token range; g^T ctx on the matrix cores, g formed from dout and seq as it is loaded, tokens ascending;
//     the partial tiles go to ws.
//   finish kernel: the partials in split order, ADDED into the caller's gradients; the session sums.
// CONCAT is two copy kernels (the session-level d ctx: a thread per element, the L rows in token order).
// No float atomics; every sum has one fixed order.
#include "../../include/t4r_hip_postfusion.h"
#include "mfma_frag.h"
#include <limits.h>

#define PF_MAX_D 1024
#define PF_MAX_C 256
#define PF_TOK 128                     // tokens per workgroup of the tile kernels (four waves of 32)
#define PF_PART_FLOATS (4l << 20)      // [d_w | d_b] partials: at most 4 Mi floats
#define PF_MAX_SPLITS 1024
#define PF_MAX_BLOCKS (1l << 20)       // grid-stride kernels
#define PF_MUL 0
#define PF_SUM 1
#define PF_CONCAT 2

static inline bool pf_dims_ok(int D, int C) { return D >= 1 && D <= PF_MAX_D && C >= 1 && C <= PF_MAX_C; }
static inline long pf_splits(long T, int D, int C) {
    long s = (T + 63) / 64, cap = PF_PART_FLOATS / ((long)D * (C + 1));       // cap >= 15 within the limits
    if (cap > PF_MAX_SPLITS) cap = PF_MAX_SPLITS;
    return s < cap ? s : cap;
}

extern "C" int t4r_post_fusion_supported(int D, int C) { return pf_dims_ok(D, C) ? 1 : 0; }

extern "C" long t4r_post_fusion_bwd_ws_floats(long ntok, int L, int D, int C, int mode, int per_session) {
    if (!pf_dims_ok(D, C) || ntok <= 0 || ntok > INT_MAX || L < 1 || ntok % L != 0) return 0;
    if (mode != PF_MUL && mode != PF_SUM) return 0;
    return (per_session ? ntok * C : 0l) + pf_splits(ntok, D, C) * D * (C + 1);
}

namespace {

struct PFArgs {
    const float* seq; const float* ctx; const float* W; const float* b; const float* dout;
    float* out; float* dseq; float* dctx; float* dW; float* db;
    float* ws_tok;                  // [T][C] per-token d ctx of a session-level context
    float* part;                    // [splits][D][C + 1]
    long T;
    int L, D, C, per_session, vec, splits, kper;
};

// p[k .. k + 3] of a row of n floats; elements past n are 0.  vec: n % 4 == 0 and the row is 16-byte aligned
__device__ __forceinline__ float4 pf_ld4(const float* p, int k, int n, bool vec) {
    if (vec) return *reinterpret_cast<const float4*>(p + k);
    float4 v;
    v.x = k < n ? p[k] : 0.f;
    v.y = k + 1 < n ? p[k + 1] : 0.f;
    v.z = k + 2 < n ? p[k + 2] : 0.f;
    v.w = k + 3 < n ? p[k + 3] : 0.f;
    return v;
}
__device__ __forceinline__ void pf_st4(float* p, int k, int n, bool vec, const float4 v) {
    if (vec) { *reinterpret_cast<float4*>(p + k) = v; return; }
    if (k < n) p[k] = v.x;
    if (k + 1 < n) p[k + 1] = v.y;
    if (k + 2 < n) p[k + 2] = v.z;
    if (k + 3 < n) p[k + 3] = v.w;
}

// acc[r] = p[d0 + xm_row(r, kh)][the lane's token]: the one place the chain is written.  crow: the token's row of ctx.
// Rows of the tile past D compute on row D - 1 of W and are never stored.  Where C is odd the last step's second slot is
// fma(0, 0, acc): it leaves every value as it is except an exact -0, which becomes +0 -- the chain "seeded with b[d], c
// ascending" is exact up to that sign of zero (the same in the forward, the backward and both access paths).
__device__ __forceinline__ void pf_proj(f32x16& acc, const PFArgs& a, int d0, const float* crow, int c, int kh, bool vec) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int d = d0 + xm_row(r, kh);
        acc[r] = a.b[d < a.D ? d : a.D - 1];
    }
    const int dw = d0 + c < a.D ? d0 + c : a.D - 1;
    const float* wrow = a.W + (long)dw * a.C;
    for (int k = 0; k < a.C; k += 4) {
        const float4 w = pf_ld4(wrow, k, a.C, vec), x = pf_ld4(crow, k, a.C, vec);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kh ? w.y : w.x, kh ? x.y : x.x, acc, 0, 0, 0);              // c = k, k + 1
        if (k + 2 < a.C) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kh ? w.w : w.z, kh ? x.w : x.z, acc, 0, 0, 0);   // k + 2, k + 3
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void pf_fwd_kernel(PFArgs a) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, kh = lane >> 5;
    const int D = a.D;
    const bool vec = a.vec != 0;
    const long t0 = (long)blockIdx.x * PF_TOK + wave * 32;
    if (t0 >= a.T) return;                                   // wave uniform; the kernel has no barrier
    const long t = t0 + c;
    const bool live = t < a.T;
    const long tc = live ? t : a.T - 1;                      // lanes past the end compute on the last row and store nothing
    const float* crow = a.ctx + (a.per_session ? (long)((int)tc / a.L) : tc) * a.C;
    const float* srow = a.seq + tc * D;
    float* orow = a.out + tc * D;
    for (int d0 = 0; d0 < D; d0 += 32) {
        f32x16 acc;
        pf_proj(acc, a, d0, crow, c, kh, vec);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d = d0 + 8 * g + 4 * kh;
            if (!live || d >= D) continue;
            const float4 s = pf_ld4(srow, d, D, vec);
            float4 o;
            if (MODE == PF_MUL) {
                o.x = __fmul_rn(s.x, __fadd_rn(1.f, acc[4 * g]));
                o.y = __fmul_rn(s.y, __fadd_rn(1.f, acc[4 * g + 1]));
                o.z = __fmul_rn(s.z, __fadd_rn(1.f, acc[4 * g + 2]));
                o.w = __fmul_rn(s.w, __fadd_rn(1.f, acc[4 * g + 3]));
            } else {
                o.x = __fadd_rn(s.x, acc[4 * g]);
                o.y = __fadd_rn(s.y, acc[4 * g + 1]);
                o.z = __fadd_rn(s.z, acc[4 * g + 2]);
                o.w = __fadd_rn(s.w, acc[4 * g + 3]);
            }
            pf_st4(orow, d, D, vec, o);
        }
    }
}

// NQ: the accumulators of d ctx (32 columns c each): NQ * 32 >= C
template <int MODE, int NQ>
__global__ __launch_bounds__(256) void pf_bwd_kernel(PFArgs a) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, kh = lane >> 5;
    const int D = a.D, C = a.C;
    const bool vec = a.vec != 0;
    const long t0 = (long)blockIdx.x * PF_TOK + wave * 32;
    if (t0 >= a.T) return;                                   // wave uniform; the kernel has no barrier
    const long t = t0 + c;
    const bool live = t < a.T;
    const long tc = live ? t : a.T - 1;
    const float* crow = a.ctx + (a.per_session ? (long)((int)tc / a.L) : tc) * C;
    const float* grow = a.dout + tc * D;
    const float* srow = MODE == PF_MUL ? a.seq + tc * D : nullptr;
    const bool want_ctx = a.dctx != nullptr;
    f32x16 o[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) o[q] = zero16();
    int ccol[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) ccol[q] = 32 * q + c < C ? 32 * q + c : C - 1;

    for (int d0 = 0; d0 < D; d0 += 32) {
        float gv[16];                                       // g[d0 + xm_row(r, kh)][the lane's token]; 0 past D and past T
        float4 go[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d = d0 + 8 * g + 4 * kh;
            const bool ok = live && d < D;
            go[g] = ok ? pf_ld4(grow, d, D, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
            float4 s = make_float4(1.f, 1.f, 1.f, 1.f);
            if (MODE == PF_MUL && ok) s = pf_ld4(srow, d, D, vec);
            if (MODE == PF_MUL) {
                gv[4 * g] = __fmul_rn(go[g].x, s.x); gv[4 * g + 1] = __fmul_rn(go[g].y, s.y);
                gv[4 * g + 2] = __fmul_rn(go[g].z, s.z); gv[4 * g + 3] = __fmul_rn(go[g].w, s.w);
            } else {
                gv[4 * g] = go[g].x; gv[4 * g + 1] = go[g].y; gv[4 * g + 2] = go[g].z; gv[4 * g + 3] = go[g].w;
            }
        }
        if (a.dseq) {
            f32x16 acc;
            if (MODE == PF_MUL) pf_proj(acc, a, d0, crow, c, kh, vec);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d = d0 + 8 * g + 4 * kh;
                if (!live || d >= D) continue;
                float4 v = go[g];
                if (MODE == PF_MUL) {
                    v.x = __fmul_rn(v.x, __fadd_rn(1.f, acc[4 * g]));
                    v.y = __fmul_rn(v.y, __fadd_rn(1.f, acc[4 * g + 1]));
                    v.z = __fmul_rn(v.z, __fadd_rn(1.f, acc[4 * g + 2]));
                    v.w = __fmul_rn(v.w, __fadd_rn(1.f, acc[4 * g + 3]));
                }
                pf_st4(a.dseq + tc * D, d, D, vec, v);
            }
        }
        if (want_ctx) {
            // dctx[token][c] += sum over the tile's d of g[token][d] W[d][c]; rows past D have g = 0 and read row D - 1
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int d = d0 + xm_row(r, kh);
                const float* wr = a.W + (long)(d < D ? d : D - 1) * C;
#pragma unroll
                for (int q = 0; q < NQ; ++q)
                    if (32 * q < C) o[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv[r], wr[ccol[q]], o[q], 0, 0, 0);
            }
        }
    }
    if (!want_ctx) return;
    float* dst = a.per_session ? a.ws_tok : a.dctx;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int cc = 32 * q + c;
        if (cc >= C) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long tr = t0 + xm_row(r, kh);
            if (tr < a.T) dst[tr * C + cc] = o[q][r];
        }
    }
}

// one wave per (64 x 64 tile of [d_w | d_b], split of the tokens): part[split][d][c] = sum over the split's tokens, ascending, of
// g[t][d] ctx[t'][c], with column C of ctx standing for 1
template <int MODE>
__global__ __launch_bounds__(64) void pf_dw_kernel(PFArgs a) {
    const int D = a.D, C = a.C, C1 = C + 1, lane = threadIdx.x, c = lane & 31, kh = lane >> 5;
    const int tilesC = (C1 + 63) >> 6;
    const int dI = (blockIdx.x / tilesC) << 6, cJ = (blockIdx.x % tilesC) << 6;
    const long k0 = (long)blockIdx.y * a.kper;
    const long k1 = k0 + a.kper < a.T ? k0 + a.kper : a.T;
    const bool d1 = dI + 32 < D, c1 = cJ + 32 < C1;                   // wave uniform: the second half of the tile exists
    const int da = min(dI + c, D - 1), db = min(dI + 32 + c, D - 1);
    const int ca = cJ + c, cb = cJ + 32 + c;                          // >= C: the ones column (past it: never stored)
    f32x16 o00 = zero16(), o01 = zero16(), o10 = zero16(), o11 = zero16();
    // sixteen tokens (eight steps) per round; the next round's operands are in flight while this round's feed the matrix cores
    struct Frag { float a0[8], a1[8], b0[8], b1[8]; };
    auto load = [&](Frag& f, long tt) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const long tk = tt + 2 * i + kh;
            const bool okt = tk < k1;
            const long tr = okt ? tk : k1 - 1;                        // every load is in bounds; a token past the split counts 0
            float va = a.dout[tr * D + da], vb = a.dout[tr * D + db];
            if (MODE == PF_MUL) {
                va = __fmul_rn(va, a.seq[tr * D + da]);
                vb = __fmul_rn(vb, a.seq[tr * D + db]);
            }
            f.a0[i] = okt ? va : 0.f;
            f.a1[i] = okt ? vb : 0.f;
            const float* crow = a.ctx + (a.per_session ? (long)((int)tr / a.L) : tr) * C;
            f.b0[i] = ca < C ? crow[ca] : 1.f;
            f.b1[i] = cb < C ? crow[cb] : 1.f;
        }
    };
    if (k0 < k1) {
        Frag cur, nxt;
        load(cur, k0);
        nxt = cur;
        for (long tt = k0; tt < k1; tt += 16) {
            if (tt + 16 < k1) load(nxt, tt + 16);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                o00 = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a0[i], cur.b0[i], o00, 0, 0, 0);
                if (c1) o01 = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a0[i], cur.b1[i], o01, 0, 0, 0);
                if (d1) o10 = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a1[i], cur.b0[i], o10, 0, 0, 0);
                if (d1 && c1) o11 = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a1[i], cur.b1[i], o11, 0, 0, 0);
            }
            cur = nxt;
        }
    }
    float* out = a.part + (long)blockIdx.y * D * C1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int d = dI + xm_row(r, kh);
        if (d < D && ca < C1) out[(long)d * C1 + ca] = o00[r];
        if (d < D && cb < C1) out[(long)d * C1 + cb] = o01[r];
        if (d + 32 < D && ca < C1) out[(long)(d + 32) * C1 + ca] = o10[r];
        if (d + 32 < D && cb < C1) out[(long)(d + 32) * C1 + cb] = o11[r];
    }
}

// element i < nW of [d_w | d_b]: its partials in split order, then one add into the caller's gradient; element nW + j: element j
// of the session-level d ctx, the L per-token rows in token order
__global__ __launch_bounds__(256) void pf_finish_kernel(PFArgs a, long nW, long nS) {
    const int C = a.C, C1 = C + 1;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nW + nS; i += (long)gridDim.x * 256) {
        if (i < nW) {
            const int d = (int)(i / C1), cc = (int)(i - (long)d * C1);
            float* dst = cc < C ? (a.dW ? a.dW + (long)d * C + cc : nullptr) : (a.db ? a.db + d : nullptr);
            if (!dst) continue;
            float s = a.part[i];
#pragma unroll 8
            for (int k = 1; k < a.splits; ++k) s += a.part[(long)k * nW + i];
            *dst += s;
        } else {
            const long j = i - nW, ses = j / C;
            const int cc = (int)(j - ses * C);
            const float* src = a.ws_tok + ses * a.L * C + cc;
            float s = src[0];
            for (int l = 1; l < a.L; ++l) s += src[(long)l * C];
            a.dctx[j] = s;
        }
    }
}

// out[t] = seq[t] | ctx[t'] in units of U floats (U = 4: 16-byte requests; D and C are multiples of 4 then)
template <int U>
__global__ __launch_bounds__(256) void pf_concat_fwd_kernel(PFArgs a) {
    const int D = a.D, C = a.C, upr = (D + C) / U;
    const long n = a.T * upr;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long t = i / upr;
        const int j = (int)(i - t * upr) * U;
        const float* src = j < D ? a.seq + t * D + j : a.ctx + (a.per_session ? (long)((int)t / a.L) : t) * C + (j - D);
        float* dst = a.out + t * (D + C) + j;
        if (U == 4) *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
        else *dst = *src;
    }
}

// dseq = dout[:, :D] (units [0, nA)), dctx = dout[:, D:] or its sum over a session's L rows in token order (units [nA, nA + nB))
template <int U>
__global__ __launch_bounds__(256) void pf_concat_bwd_kernel(PFArgs a, long nA, long nB) {
    const int D = a.D, C = a.C, W = D + C, du = D / U, cu = C / U;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nA + nB; i += (long)gridDim.x * 256) {
        if (i < nA) {
            const long t = i / du;
            const int j = (int)(i - t * du) * U;
            if (U == 4) *reinterpret_cast<float4*>(a.dseq + t * D + j) = *reinterpret_cast<const float4*>(a.dout + t * W + j);
            else a.dseq[t * D + j] = a.dout[t * W + j];
            continue;
        }
        const long e = i - nA, row = e / cu;
        const int j = (int)(e - row * cu) * U;
        const int nl = a.per_session ? a.L : 1;
        const float* src = a.dout + row * nl * W + D + j;
        if (U == 4) {
            float4 s = *reinterpret_cast<const float4*>(src);
            for (int l = 1; l < nl; ++l) {
                const float4 v = *reinterpret_cast<const float4*>(src + (long)l * W);
                s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            }
            *reinterpret_cast<float4*>(a.dctx + row * C + j) = s;
        } else {
            float s = src[0];
            for (int l = 1; l < nl; ++l) s += src[(long)l * W];
            a.dctx[row * C + j] = s;
        }
    }
}

}  // namespace

#define PF_A4(p) ((uintptr_t)(p) % 4 == 0)
#define PF_A16(p) ((uintptr_t)(p) % 16 == 0)
// the sizes both directions share: checked first, and nothing is dereferenced
#define PF_CHECK_DIMS(name)                                                                                   \
    T4R_CHECK_ARG(D >= 1 && D <= PF_MAX_D, name ": 1 <= D <= 1024");                                          \
    T4R_CHECK_ARG(C >= 1 && C <= PF_MAX_C, name ": 1 <= C <= 256 context columns");                           \
    T4R_CHECK_ARG(ntok >= 0 && ntok <= INT_MAX, name ": 0 <= ntok < 2^31");                                   \
    T4R_CHECK_ARG(L >= 1 && ntok % L == 0, name ": L must be >= 1 and divide ntok");                          \
    T4R_CHECK_ARG(mode == PF_MUL || mode == PF_SUM || mode == PF_CONCAT, name ": mode must be 0 (mul), 1 (sum) or 2 (concat)"); \
    T4R_CHECK_ARG(mode != PF_CONCAT || (!W && !b), name ": concat has no parameters: W and b must be NULL");  \
    if (ntok == 0) return 0

static inline unsigned pf_blocks(long n) {
    const long b = (n + 255) / 256;
    return (unsigned)(b < PF_MAX_BLOCKS ? b : PF_MAX_BLOCKS);
}

extern "C" int t4r_post_fusion_fwd(void* stream, const float* seq, const float* ctx, const float* W, const float* b, float* out,
                                   long ntok, int L, int D, int C, int mode, int per_session) {
    PF_CHECK_DIMS("post_fusion_fwd");
    T4R_CHECK_ARG(seq && ctx && out, "post_fusion_fwd: null pointer (seq, ctx or out)");
    T4R_CHECK_ARG(mode == PF_CONCAT || (W && b), "post_fusion_fwd: null pointer (W or b)");
    T4R_CHECK_ARG(PF_A4(seq) && PF_A4(ctx) && PF_A4(W) && PF_A4(b) && PF_A4(out),
                  "post_fusion_fwd: every pointer must be 4-byte aligned");
    PFArgs a = {};
    a.seq = seq; a.ctx = ctx; a.W = W; a.b = b; a.out = out; a.T = ntok; a.L = L; a.D = D; a.C = C;
    a.per_session = per_session ? 1 : 0;
    a.vec = D % 4 == 0 && C % 4 == 0 && PF_A16(seq) && PF_A16(ctx) && PF_A16(W) && PF_A16(out);
    hipStream_t st = (hipStream_t)stream;
    if (mode == PF_CONCAT) {
        if (a.vec) hipLaunchKernelGGL(pf_concat_fwd_kernel<4>, dim3(pf_blocks(ntok * ((D + C) / 4))), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(pf_concat_fwd_kernel<1>, dim3(pf_blocks(ntok * (D + C))), dim3(256), 0, st, a);
    } else {
        const dim3 grid((unsigned)((ntok + PF_TOK - 1) / PF_TOK));
        if (mode == PF_MUL) hipLaunchKernelGGL(pf_fwd_kernel<PF_MUL>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(pf_fwd_kernel<PF_SUM>, grid, dim3(256), 0, st, a);
    }
    T4R_LAUNCH_CHECK();
    return 0;
}

template <int MODE>
static void pf_launch_bwd_tile(const PFArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)((a.T + PF_TOK - 1) / PF_TOK));
    if (a.C <= 32) hipLaunchKernelGGL((pf_bwd_kernel<MODE, 1>), grid, dim3(256), 0, st, a);
    else if (a.C <= 64) hipLaunchKernelGGL((pf_bwd_kernel<MODE, 2>), grid, dim3(256), 0, st, a);
    else if (a.C <= 128) hipLaunchKernelGGL((pf_bwd_kernel<MODE, 4>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((pf_bwd_kernel<MODE, 8>), grid, dim3(256), 0, st, a);
}

extern "C" int t4r_post_fusion_bwd(void* stream, const float* dout, const float* seq, const float* ctx, const float* W,
                                   const float* b, float* dseq, float* dctx, float* d_w, float* d_b, float* ws, long ntok, int L,
                                   int D, int C, int mode, int per_session) {
    PF_CHECK_DIMS("post_fusion_bwd");
    T4R_CHECK_ARG(mode != PF_CONCAT || (!d_w && !d_b), "post_fusion_bwd: concat has no parameters: d_w and d_b must be NULL");
    T4R_CHECK_ARG(dout, "post_fusion_bwd: null pointer (dout)");
    T4R_CHECK_ARG(mode == PF_CONCAT || (ctx && W && b), "post_fusion_bwd: null pointer (ctx, W or b)");
    T4R_CHECK_ARG(mode != PF_MUL || seq, "post_fusion_bwd: null pointer (seq)");
    const bool want_w = d_w || d_b;
    const bool ses_ws = mode != PF_CONCAT && per_session && dctx;
    T4R_CHECK_ARG(ws || !(want_w || ses_ws), "post_fusion_bwd: null pointer (ws)");
    T4R_CHECK_ARG(PF_A4(dout) && PF_A4(seq) && PF_A4(ctx) && PF_A4(W) && PF_A4(b) && PF_A4(dseq) && PF_A4(dctx) && PF_A4(d_w)
                      && PF_A4(d_b) && PF_A4(ws),
                  "post_fusion_bwd: every pointer must be 4-byte aligned");
    PFArgs a = {};
    a.dout = dout; a.seq = seq; a.ctx = ctx; a.W = W; a.b = b; a.dseq = dseq; a.dctx = dctx; a.dW = d_w; a.db = d_b;
    a.T = ntok; a.L = L; a.D = D; a.C = C;
    a.per_session = per_session ? 1 : 0;
    a.vec = D % 4 == 0 && C % 4 == 0 && PF_A16(dout) && PF_A16(seq) && PF_A16(ctx) && PF_A16(W) && PF_A16(dseq) && PF_A16(dctx);
    hipStream_t st = (hipStream_t)stream;
    if (mode == PF_CONCAT) {
        if (!dseq && !dctx) return 0;
        const int U = a.vec ? 4 : 1;
        const long nA = dseq ? ntok * (D / U) : 0;
        const long nB = dctx ? (per_session ? ntok / L : ntok) * (C / U) : 0;
        if (a.vec) hipLaunchKernelGGL(pf_concat_bwd_kernel<4>, dim3(pf_blocks(nA + nB)), dim3(256), 0, st, a, nA, nB);
        else hipLaunchKernelGGL(pf_concat_bwd_kernel<1>, dim3(pf_blocks(nA + nB)), dim3(256), 0, st, a, nA, nB);
        T4R_LAUNCH_CHECK();
        return 0;
    }
    a.ws_tok = ws;
    a.part = ws ? ws + (per_session ? ntok * C : 0l) : nullptr;
    a.splits = (int)pf_splits(ntok, D, C);
    const long kper = (ntok + a.splits - 1) / a.splits;
    a.kper = (int)(kper + (kper & 1));
    if (dseq || dctx) {
        if (mode == PF_MUL) pf_launch_bwd_tile<PF_MUL>(a, st);
        else pf_launch_bwd_tile<PF_SUM>(a, st);
        T4R_LAUNCH_CHECK();
    }
    if (want_w) {
        const int tiles = ((D + 63) / 64) * ((C + 1 + 63) / 64);
        const dim3 grid((unsigned)tiles, (unsigned)a.splits);
        if (mode == PF_MUL) hipLaunchKernelGGL(pf_dw_kernel<PF_MUL>, grid, dim3(64), 0, st, a);
        else hipLaunchKernelGGL(pf_dw_kernel<PF_SUM>, grid, dim3(64), 0, st, a);
        T4R_LAUNCH_CHECK();
    }
    const long nW = want_w ? (long)D * (C + 1) : 0;
    const long nS = ses_ws ? (ntok / L) * C : 0;
    if (nW + nS > 0) {
        hipLaunchKernelGGL(pf_finish_kernel, dim3(pf_blocks(nW + nS)), dim3(256), 0, st, a, nW, nS);
        T4R_LAUNCH_CHECK();
    }
    return 0;
}
