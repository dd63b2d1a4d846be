// MLP block (include/t4r_hip_mlpblock.h): a stack of 1 .. 4 layers a_i = dropout(relu(b_i + W_i a_{i-1})) per token, and the
// backward of all of it.  gfx950 only.
//
// Forward, one launch.  A workgroup is ONE wave and owns 32 consecutive tokens, the token on the lane (mfma_frag.h's map: lane
// (c, kh) holds rows xm_row(r, kh) of column c -- the token -- of a 32 x 32 tile in its 16 accumulator registers).  Per layer it
// walks the output width in groups of up to four 32-row tiles and forms z^T = W a^T on the fp32 matrix cores
// (v_mfma_f32_32x32x2_f32: bit for bit one fp32 fma chain per element, seeded with b[d]).  Step s of the contraction takes
// k = 2 s + kh, so the chain runs over k ASCENDING in every layer.  Layer 0 reads its B operand from the token's row of x
// (four consecutive floats per request, elements (0, 2) or (1, 3) by lane half); a later layer reads it from the wave's own
// tile of a_{i-1} in LDS, stored [k][token] with pitch 32: the read of row 2 s + kh and the write of rows r, r + 4 by the two
// lane halves are conflict free (32 banks per half).  Two LDS buffers alternate between the layers; the last layer's output
// goes to memory only, and so does every a_i where the caller asks for them (training).  A token's chains see only its own row.
// Backward, chain kernel (one launch): the same wave-per-32-tokens form.  dz_i = da_i gate_i in the accumulator's image goes to
// LDS [d][token] and to the workspace rows the weight gradients read; da_{i-1}^T = W_i^T dz_i^T runs over d ASCENDING with the A
// operand a 128-byte coalesced row segment of W_i per step; its accumulator image is again "token on the lane", which is what
// the gate of layer i - 1 (a_{i-1} > 0, or the recomputed keep mask) and the next product want: no exchange but the LDS tile.
// d W kernel: one wave per 64 x 64 tile of [d W_i | d b_i] ([N_i, K_i + 1]: d b is the product with a column of ones) of every
// layer and per split of the token range, tokens ascending; partial tiles to the workspace.  Finish kernel: the partials in
// split order, ADDED into the caller's gradients.  No float atomics; every sum has one fixed order.
#include "../../include/t4r_hip_mlpblock.h"
#include "mfma_frag.h"
#include <limits.h>

#define ML_MAX_LAYERS 4
#define ML_MAX_K0 1024
#define ML_MAX_N 512
#define ML_SITE 8                      // T4R_SITE_MLP_BLOCK: the dropout site of this block (layer byte = the layer's index)
#define ML_PART_FLOATS (8l << 20)      // [d W | d b] partials of all layers: at most 8 Mi floats
#define ML_MAX_SPLITS 1024
#define ML_MAX_BLOCKS (1l << 20)       // grid-stride kernels

extern "C" unsigned long long t4r_dropout_ctr_hi(unsigned long long offset, int layer, int site);

static inline bool ml_dims_ok(int n, int K0, const int* N) {
    if (n < 1 || n > ML_MAX_LAYERS || !N || K0 < 1 || K0 > ML_MAX_K0) return false;
    for (int i = 0; i < n; ++i)
        if (N[i] < 1 || N[i] > ML_MAX_N) return false;
    return true;
}
// floats of one split's partials over all layers
static inline long ml_part_floats(int n, int K0, const int* N) {
    long s = 0;
    for (int i = 0; i < n; ++i) s += (long)N[i] * ((i ? N[i - 1] : K0) + 1);
    return s;
}
static inline long ml_splits(long T, long part) {
    long s = (T + 63) / 64, cap = ML_PART_FLOATS / part;                      // cap >= 6 within the limits
    if (cap > ML_MAX_SPLITS) cap = ML_MAX_SPLITS;
    return s < cap ? s : cap;
}
static inline long ml_round4(long v) { return (v + 3) & ~3l; }

extern "C" int t4r_mlp_stack_supported(int n, int K0, const int* N) { return ml_dims_ok(n, K0, N) ? 1 : 0; }

extern "C" long t4r_mlp_stack_bwd_ws_floats(long ntok, int n, int K0, const int* N) {
    if (!ml_dims_ok(n, K0, N) || ntok <= 0 || ntok > INT_MAX) return 0;
    long rows = 0;
    for (int i = 0; i < n; ++i) rows += ml_round4(ntok * N[i]);
    const long part = ml_part_floats(n, K0, N);
    return rows + ml_splits(ntok, part) * part;
}

namespace {

struct MLArgs {
    const float* x; const float* dout;
    const float* W[ML_MAX_LAYERS]; const float* b[ML_MAX_LAYERS];
    float* acts[ML_MAX_LAYERS];     // forward: where a_i is stored (null: nowhere); backward: read
    float* dz[ML_MAX_LAYERS];       // backward: [T][N_i] rows for the weight gradients (null: not wanted)
    float* dx;
    float* dW[ML_MAX_LAYERS]; float* db[ML_MAX_LAYERS];
    float* part;                    // [layer: part_off][splits][N_i][K_i + 1]
    long part_off[ML_MAX_LAYERS];
    long T;
    int n, K[ML_MAX_LAYERS], N[ML_MAX_LAYERS];
    int tile_end[ML_MAX_LAYERS];    // d W kernel: running count of 64 x 64 tiles up to and including layer i
    int vin, vout, vdx;             // bit i: 16-byte requests for layer i's operand rows / stored rows; vdx: for dx
    int relu, buf_floats, splits, kper;
    DropCfg drop[ML_MAX_LAYERS];
};

// p[k .. k + 3] of a row of n floats; elements past n are 0.  vec: n % 4 == 0 and the row is 16-byte aligned
__device__ __forceinline__ float4 ml_ld4(const float* p, int k, int n, bool vec) {
    if (vec) return *reinterpret_cast<const float4*>(p + k);
    float4 v;
    v.x = k < n ? p[k] : 0.f;
    v.y = k + 1 < n ? p[k + 1] : 0.f;
    v.z = k + 2 < n ? p[k + 2] : 0.f;
    v.w = k + 3 < n ? p[k + 3] : 0.f;
    return v;
}
__device__ __forceinline__ void ml_st4(float* p, int k, int n, bool vec, const float4 v) {
    if (vec) { *reinterpret_cast<float4*>(p + k) = v; return; }
    if (k < n) p[k] = v.x;
    if (k + 1 < n) p[k + 1] = v.y;
    if (k + 2 < n) p[k + 2] = v.z;
    if (k + 3 < n) p[k + 3] = v.w;
}
// the dropout factors of elements (t, d .. d + 3) of a [T, N] site; elements past N get 0
__device__ __forceinline__ float4 ml_drop4(const DropCfg& dc, long t, int d, int N) {
    const unsigned long long idx = (unsigned long long)t * (unsigned long long)N + (unsigned long long)d;
    if ((N & 3) == 0) return drop_scale4(dc, idx);          // d % 4 == 0: the four elements are one Philox block
    float4 m;
    m.x = drop_scale(dc, idx);
    m.y = d + 1 < N ? drop_scale(dc, idx + 1) : 0.f;
    m.z = d + 2 < N ? drop_scale(dc, idx + 2) : 0.f;
    m.w = d + 3 < N ? drop_scale(dc, idx + 3) : 0.f;
    return m;
}
// rows d .. d + 3 (those below N) of column c of a [N][32] LDS tile
__device__ __forceinline__ void ml_lds_put4(float* tile, int d, int N, int c, const float4 v) {
    tile[d * 32 + c] = v.x;
    if (d + 1 < N) tile[(d + 1) * 32 + c] = v.y;
    if (d + 2 < N) tile[(d + 2) * 32 + c] = v.z;
    if (d + 3 < N) tile[(d + 3) * 32 + c] = v.w;
}

__global__ __launch_bounds__(64) void ml_fwd_kernel(MLArgs a) {
    extern __shared__ float ml_lds[];
    const int lane = threadIdx.x, c = lane & 31, kh = lane >> 5;
    const long t = (long)blockIdx.x * 32 + c;
    const bool live = t < a.T;
    const long tc = live ? t : a.T - 1;                      // lanes past the end compute on the last row and store nothing
    for (int i = 0; i < a.n; ++i) {
        const int K = a.K[i], N = a.N[i];
        const bool vin = (a.vin >> i) & 1, vout = (a.vout >> i) & 1;
        const float* xrow = a.x + tc * K;                                      // layer 0 only
        const float* lin = ml_lds + ((i + 1) & 1) * a.buf_floats;              // a_{i-1} [K][32]
        float* lout = ml_lds + (i & 1) * a.buf_floats;                         // a_i [N][32]
        const bool hand = i + 1 < a.n;
        float* orow = a.acts[i] ? a.acts[i] + tc * N : nullptr;
        const float* W = a.W[i];
        const float* bias = a.b[i];
        const bool dropping = a.drop[i].p > 0.f;
        for (int d0 = 0; d0 < N; d0 += 128) {
            f32x16 acc[4];
            const float* wrow[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int dw = d0 + 32 * q + c;
                wrow[q] = W + (long)(dw < N ? dw : N - 1) * K;                // rows past N compute on row N - 1, never stored
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int d = d0 + 32 * q + xm_row(r, kh);
                    acc[q][r] = bias ? bias[d < N ? d : N - 1] : 0.f;
                }
            }
            for (int k = 0; k < K; k += 4) {
                float x0, x1;                                                  // a_{i-1}[token][k + kh], [k + 2 + kh]
                if (i == 0) {
                    const float4 xv = ml_ld4(xrow, k, K, vin);
                    x0 = kh ? xv.y : xv.x; x1 = kh ? xv.w : xv.z;
                } else {
                    x0 = k + kh < K ? lin[(k + kh) * 32 + c] : 0.f;
                    x1 = k + 2 + kh < K ? lin[(k + 2 + kh) * 32 + c] : 0.f;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (d0 + 32 * q >= N) continue;                            // wave uniform
                    const float4 w = ml_ld4(wrow[q], k, K, vin);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(kh ? w.y : w.x, x0, acc[q], 0, 0, 0);           // k, k + 1
                    if (k + 2 < K) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(kh ? w.w : w.z, x1, acc[q], 0, 0, 0);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int d = d0 + 32 * q + 8 * g + 4 * kh;
                    if (d >= N) continue;
                    float4 v = make_float4(acc[q][4 * g], acc[q][4 * g + 1], acc[q][4 * g + 2], acc[q][4 * g + 3]);
                    if (a.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
                    if (dropping) {
                        const float4 m = ml_drop4(a.drop[i], tc, d, N);
                        v.x = __fmul_rn(v.x, m.x); v.y = __fmul_rn(v.y, m.y); v.z = __fmul_rn(v.z, m.z); v.w = __fmul_rn(v.w, m.w);
                    }
                    if (hand) ml_lds_put4(lout, d, N, c, v);
                    if (orow && live) ml_st4(orow, d, N, vout, v);
                }
            }
        }
        if (hand) __syncthreads();                                             // one wave: orders the tile's writes before its reads
    }
}

// dz_j[t][d .. d + 3] = da * gate_j for the lane's token: to the LDS tile (where the next product reads it) and to the workspace
__device__ __forceinline__ void ml_gate_emit(const MLArgs& a, int j, long tc, bool live, int c, int d, float4 da, float* tile,
                                             bool want_tile) {
    const int N = a.N[j];
    const bool vec = (a.vout >> j) & 1;
    float4 g = make_float4(1.f, 1.f, 1.f, 1.f);
    if (a.relu) {
        const float4 av = ml_ld4(a.acts[j] + tc * N, d, N, vec);
        const float s = a.drop[j].inv_keep;
        g = make_float4(av.x > 0.f ? s : 0.f, av.y > 0.f ? s : 0.f, av.z > 0.f ? s : 0.f, av.w > 0.f ? s : 0.f);
    } else if (a.drop[j].p > 0.f) {
        g = ml_drop4(a.drop[j], tc, d, N);
    }
    float4 dz;
    dz.x = __fmul_rn(da.x, g.x); dz.y = __fmul_rn(da.y, g.y); dz.z = __fmul_rn(da.z, g.z); dz.w = __fmul_rn(da.w, g.w);
    if (want_tile) ml_lds_put4(tile, d, N, c, dz);
    if (a.dz[j] && live) ml_st4(a.dz[j] + tc * N, d, N, vec, dz);
}

__global__ __launch_bounds__(64) void ml_bwd_kernel(MLArgs a) {
    extern __shared__ float ml_lds[];
    const int lane = threadIdx.x, c = lane & 31, kh = lane >> 5;
    const long t = (long)blockIdx.x * 32 + c;
    const bool live = t < a.T;
    const long tc = live ? t : a.T - 1;
    {   // the last layer's dz from dout
        const int j = a.n - 1, N = a.N[j];
        const bool vec = (a.vout >> j) & 1;
        const bool want_tile = j > 0 || a.dx;
        float* tile = ml_lds + (j & 1) * a.buf_floats;
        for (int d = 4 * kh; d < N; d += 8)
            ml_gate_emit(a, j, tc, live, c, d, ml_ld4(a.dout + tc * N, d, N, vec), tile, want_tile);
        __syncthreads();
    }
    for (int i = a.n - 1; i >= 0; --i) {
        if (i == 0 && !a.dx) break;
        // da_{i-1}[token][k] = sum_d dz_i[token][d] W_i[d][k], d ascending (step s: d = 2 s + kh)
        const int K = a.K[i], N = a.N[i];
        const float* tin = ml_lds + (i & 1) * a.buf_floats;                    // dz_i [N][32]
        float* tout = ml_lds + ((i + 1) & 1) * a.buf_floats;                   // dz_{i-1} [K][32]
        const float* W = a.W[i];
        const bool want_tile = i > 1 || (i == 1 && a.dx);
        for (int k0 = 0; k0 < K; k0 += 128) {
            f32x16 acc[4];
            int col[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc[q] = zero16();
                const int kc = k0 + 32 * q + c;
                col[q] = kc < K ? kc : K - 1;                                  // columns past K compute on column K - 1, never stored
            }
            for (int d = 0; d < N; d += 2) {
                const bool ok = d + kh < N;                                    // N odd: the last step's second slot is fma(0, 0, acc)
                const float g = ok ? tin[(d + kh) * 32 + c] : 0.f;
                const float* wr = W + (long)(ok ? d + kh : N - 1) * K;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (k0 + 32 * q >= K) continue;                            // wave uniform
                    const float w = ok ? wr[col[q]] : 0.f;
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(w, g, acc[q], 0, 0, 0);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int k = k0 + 32 * q + 8 * g + 4 * kh;
                    if (k >= K) continue;
                    const float4 v = make_float4(acc[q][4 * g], acc[q][4 * g + 1], acc[q][4 * g + 2], acc[q][4 * g + 3]);
                    if (i > 0) ml_gate_emit(a, i - 1, tc, live, c, k, v, tout, want_tile);
                    else if (live) ml_st4(a.dx + tc * K, k, K, a.vdx != 0, v);
                }
            }
        }
        __syncthreads();
    }
}

// one wave per (64 x 64 tile of [d W_i | d b_i], split of the tokens): part[split][d][k] = sum over the split's tokens, ascending,
// of dz_i[t][d] a_{i-1}[t][k], with column K of a_{i-1} standing for 1
__global__ __launch_bounds__(64) void ml_dw_kernel(MLArgs a) {
    int li = 0;
    while (li + 1 < a.n && (int)blockIdx.x >= a.tile_end[li]) ++li;
    const int tile = (int)blockIdx.x - (li ? a.tile_end[li - 1] : 0);
    const int D = a.N[li], C = a.K[li], C1 = C + 1, lane = threadIdx.x, c = lane & 31, kh = lane >> 5;
    const float* gsrc = a.dz[li];
    const float* prev = li ? a.acts[li - 1] : a.x;
    const int tilesC = (C1 + 63) >> 6;
    const int dI = (tile / tilesC) << 6, cJ = (tile % tilesC) << 6;
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
            f.a0[i] = okt ? gsrc[tr * D + da] : 0.f;
            f.a1[i] = okt ? gsrc[tr * D + db] : 0.f;
            const float* prow = prev + tr * C;
            f.b0[i] = ca < C ? prow[ca] : 1.f;
            f.b1[i] = cb < C ? prow[cb] : 1.f;
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
    float* out = a.part + a.part_off[li] + (long)blockIdx.y * D * C1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int d = dI + xm_row(r, kh);
        if (d < D && ca < C1) out[(long)d * C1 + ca] = o00[r];
        if (d < D && cb < C1) out[(long)d * C1 + cb] = o01[r];
        if (d + 32 < D && ca < C1) out[(long)(d + 32) * C1 + ca] = o10[r];
        if (d + 32 < D && cb < C1) out[(long)(d + 32) * C1 + cb] = o11[r];
    }
}

// element e of layer li's [d W | d b]: its partials in split order, then one add into the caller's gradient
__global__ __launch_bounds__(256) void ml_finish_kernel(MLArgs a, long total) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        int li = 0;
        long e = i;
        while (li + 1 < a.n && e >= (long)a.N[li] * (a.K[li] + 1)) { e -= (long)a.N[li] * (a.K[li] + 1); ++li; }
        if (!a.dz[li]) continue;                                      // this layer's gradients are not asked for
        const int C = a.K[li], C1 = C + 1;
        const long nW = (long)a.N[li] * C1;
        const int d = (int)(e / C1), cc = (int)(e - (long)d * C1);
        float* dst = cc < C ? (a.dW[li] ? a.dW[li] + (long)d * C + cc : nullptr) : (a.db[li] ? a.db[li] + d : nullptr);
        if (!dst) continue;
        const float* p = a.part + a.part_off[li];
        float s = p[e];
#pragma unroll 8
        for (int k = 1; k < a.splits; ++k) s += p[(long)k * nW + e];
        *dst += s;
    }
}

}  // namespace

#define ML_A4(p) ((uintptr_t)(p) % 4 == 0)
#define ML_A16(p) ((uintptr_t)(p) % 16 == 0)
// the sizes both directions share: checked first, and nothing is dereferenced but the host array N
#define ML_CHECK_DIMS(name)                                                                                   \
    T4R_CHECK_ARG(n >= 1 && n <= ML_MAX_LAYERS, name ": 1 <= n <= 4 layers");                                 \
    T4R_CHECK_ARG(N, name ": null pointer (N)");                                                              \
    T4R_CHECK_ARG(K0 >= 1 && K0 <= ML_MAX_K0, name ": 1 <= K0 <= 1024");                                      \
    for (int i_ = 0; i_ < n; ++i_) T4R_CHECK_ARG(N[i_] >= 1 && N[i_] <= ML_MAX_N, name ": 1 <= N[i] <= 512"); \
    T4R_CHECK_ARG(ntok >= 0 && ntok <= INT_MAX, name ": 0 <= ntok < 2^31");                                   \
    T4R_CHECK_ARG(relu == 0 || relu == 1, name ": relu must be 0 or 1");                                      \
    T4R_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, name ": 0 <= drop_p < 1");                                   \
    if (ntok == 0) return 0

static void ml_fill_dims(MLArgs& a, long ntok, int n, int K0, const int* N, int relu, float drop_p, unsigned long long seed,
                         unsigned long long offset) {
    a.T = ntok; a.n = n; a.relu = relu;
    for (int i = 0; i < ML_MAX_LAYERS; ++i) {
        const int j = i < n ? i : n - 1;                               // unused slots repeat the last layer: no field is left unset
        a.K[i] = j ? N[j - 1] : K0;
        a.N[i] = N[j];
        a.drop[i] = make_drop(drop_p, seed, t4r_dropout_ctr_hi(offset, j, ML_SITE));
    }
}

extern "C" int t4r_mlp_stack_fwd(void* stream, const float* x, const float* const* W, const float* const* b, float* const* acts,
                                 float* out, long ntok, int n, int K0, const int* N, int relu, float drop_p,
                                 unsigned long long seed, unsigned long long offset) {
    ML_CHECK_DIMS("mlp_stack_fwd");
    T4R_CHECK_ARG(x && W, "mlp_stack_fwd: null pointer (x or W)");
    T4R_CHECK_ARG(acts || out, "mlp_stack_fwd: null pointer (out, with no acts)");
    T4R_CHECK_ARG(ML_A4(x) && ML_A4(out), "mlp_stack_fwd: every pointer must be 4-byte aligned");
    MLArgs a = {};
    ml_fill_dims(a, ntok, n, K0, N, relu, drop_p, seed, offset);
    a.x = x;
    for (int i = 0; i < n; ++i) {
        T4R_CHECK_ARG(W[i], "mlp_stack_fwd: null pointer (W[i])");
        T4R_CHECK_ARG(!acts || acts[i], "mlp_stack_fwd: null pointer (acts[i])");
        a.W[i] = W[i];
        a.b[i] = b ? b[i] : nullptr;
        a.acts[i] = acts ? acts[i] : (i == n - 1 ? out : nullptr);
        T4R_CHECK_ARG(ML_A4(a.W[i]) && ML_A4(a.b[i]) && ML_A4(a.acts[i]), "mlp_stack_fwd: every pointer must be 4-byte aligned");
        if (a.K[i] % 4 == 0 && ML_A16(a.W[i]) && (i > 0 || ML_A16(x))) a.vin |= 1 << i;
        if (a.N[i] % 4 == 0 && ML_A16(a.acts[i])) a.vout |= 1 << i;
        if (i + 1 < n && a.N[i] * 32 > a.buf_floats) a.buf_floats = a.N[i] * 32;
    }
    T4R_CHECK_ARG(!acts || !out || out == acts[n - 1], "mlp_stack_fwd: with acts, out must be NULL or acts[n - 1]");
    const size_t smem = (size_t)(n > 2 ? 2 : 1) * a.buf_floats * sizeof(float);       // <= 128 KiB
    static T4rLdsAttr attr;
    t4r_ensure_dynamic_lds((const void*)ml_fwd_kernel, smem, attr);
    hipLaunchKernelGGL(ml_fwd_kernel, dim3((unsigned)((ntok + 31) / 32)), dim3(64), smem, (hipStream_t)stream, a);
    T4R_LAUNCH_CHECK();
    return 0;
}

extern "C" int t4r_mlp_stack_bwd(void* stream, const float* dout, const float* x, const float* const* W, const float* const* acts,
                                 float* dx, float* const* d_W, float* const* d_b, float* ws, long ntok, int n, int K0, const int* N,
                                 int relu, float drop_p, unsigned long long seed, unsigned long long offset) {
    ML_CHECK_DIMS("mlp_stack_bwd");
    T4R_CHECK_ARG(dout && W, "mlp_stack_bwd: null pointer (dout or W)");
    T4R_CHECK_ARG(ML_A4(dout) && ML_A4(x) && ML_A4(dx) && ML_A4(ws), "mlp_stack_bwd: every pointer must be 4-byte aligned");
    MLArgs a = {};
    ml_fill_dims(a, ntok, n, K0, N, relu, drop_p, seed, offset);
    a.x = x; a.dout = dout; a.dx = dx;
    a.vdx = K0 % 4 == 0 && ML_A16(dx);
    bool want_w = false;
    long off = 0, tiles = 0;
    const long part = ml_part_floats(n, K0, N);
    a.splits = (int)ml_splits(ntok, part);
    for (int i = 0; i < n; ++i) {
        T4R_CHECK_ARG(W[i], "mlp_stack_bwd: null pointer (W[i])");
        a.W[i] = W[i];
        a.acts[i] = acts ? const_cast<float*>(acts[i]) : nullptr;
        a.dW[i] = d_W ? d_W[i] : nullptr;
        a.db[i] = d_b ? d_b[i] : nullptr;
        const bool want = a.dW[i] || a.db[i];
        T4R_CHECK_ARG(!relu || a.acts[i], "mlp_stack_bwd: null pointer (acts[i], read by the ReLU gate)");
        T4R_CHECK_ARG(!want || (i ? (acts && acts[i - 1]) : x != nullptr),
                      "mlp_stack_bwd: null pointer (the input of a layer whose weight gradient is asked for)");
        T4R_CHECK_ARG(ML_A4(a.W[i]) && ML_A4(a.acts[i]) && ML_A4(a.dW[i]) && ML_A4(a.db[i]),
                      "mlp_stack_bwd: every pointer must be 4-byte aligned");
        float* rows = ws + off;
        off += ml_round4(ntok * a.N[i]);
        a.dz[i] = want ? rows : nullptr;
        if (a.N[i] % 4 == 0 && ML_A16(rows) && (!relu || ML_A16(a.acts[i])) && (i + 1 < n || ML_A16(dout))) a.vout |= 1 << i;
        if (want) tiles += (long)((a.N[i] + 63) / 64) * ((a.K[i] + 1 + 63) / 64);
        a.tile_end[i] = (int)tiles;
        if (a.N[i] * 32 > a.buf_floats) a.buf_floats = a.N[i] * 32;
        want_w = want_w || want;
    }
    for (int i = n; i < ML_MAX_LAYERS; ++i) a.tile_end[i] = (int)tiles;
    T4R_CHECK_ARG(ws || !want_w, "mlp_stack_bwd: null pointer (ws)");
    a.part = ws + off;
    off = 0;
    for (int i = 0; i < n; ++i) {
        a.part_off[i] = off;
        off += (long)a.splits * a.N[i] * (a.K[i] + 1);
    }
    const long kper = (ntok + a.splits - 1) / a.splits;
    a.kper = (int)(kper + (kper & 1));
    hipStream_t st = (hipStream_t)stream;
    if (!dx && !want_w) return 0;
    {
        const size_t smem = (size_t)(n > 1 ? 2 : 1) * a.buf_floats * sizeof(float);   // <= 128 KiB
        static T4rLdsAttr attr;
        t4r_ensure_dynamic_lds((const void*)ml_bwd_kernel, smem, attr);
        hipLaunchKernelGGL(ml_bwd_kernel, dim3((unsigned)((ntok + 31) / 32)), dim3(64), smem, st, a);
        T4R_LAUNCH_CHECK();
    }
    if (want_w) {
        hipLaunchKernelGGL(ml_dw_kernel, dim3((unsigned)tiles, (unsigned)a.splits), dim3(64), 0, st, a);
        T4R_LAUNCH_CHECK();
        const long b = (part + 255) / 256;
        hipLaunchKernelGGL(ml_finish_kernel, dim3((unsigned)(b < ML_MAX_BLOCKS ? b : ML_MAX_BLOCKS)), dim3(256), 0, st, a, part);
        T4R_LAUNCH_CHECK();
    }
    return 0;
}
