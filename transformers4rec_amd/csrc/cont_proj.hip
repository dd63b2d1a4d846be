// Continuous-feature projection, first layer (include/t4r_hip_contproj.h): y[t][p] = relu(b[p] + sum_c w[p][c] * x_c[t]) over
// the C separate continuous columns of the batch, forward and the parameter gradients.  gfx950 only.
//
// The contraction length is the number of continuous columns (1 .. 64): too short for the matrix cores and their K alignment,
// and the operand [T, C] does not exist in memory -- each column is its own tensor, [B, L] or (a per-session feature) [B].
// Both directions tile the outputs as 64 tokens x PT columns (PT = 64 or 128) per workgroup of 256 threads.  A workgroup
// stages its PT rows of W once, transposed ([C][PT] in LDS, so that the four weights of four consecutive outputs are one
// ds_read_b128), then walks its token tiles: the C columns' 64 values go to LDS ([C][64], coalesced reads), and thread
// (row group g, column quad q) computes R = PT / 16 consecutive tokens x 4 consecutive outputs with one weight read and R
// token reads per column.  Every output is ONE chain acc = b; acc = fmaf(w[p][c], x_c, acc) for c = 0, 1, ...: the same bits in
// the forward, in the backward's recomputation, and wherever the token sits in the launch.
//
// Backward, two launches.  (1) per (token chunk, PT outputs): recompute the pre-activation with the forward's function, mask
// the incoming gradient (zero where the output is not > 0), leave it in LDS as [64][PT], and let thread (p, column group)
// add g[t][p] * x_c[t] over the tile's tokens in token order into registers; after the chunk's last tile the partial
// [PT][C + 1] (the last column is d b) goes to the workspace.  (2) the partials in chunk order, then one add into the
// caller's gradients (sixteen groups of chunks, each in chunk order, then the groups in order).  No atomics.
#include "t4r_common.h"
#include <limits.h>

#define CP_MAX_C 64
#define CP_MAX_P 1024
#define CP_TOK 64                // tokens per tile
#define CP_MAX_CHUNKS 512        // token chunks of the backward (= workgroups along the tokens)
#define CP_FWD_WGS 2048          // workgroups along the tokens of the forward

static inline bool cp_dims_ok(int C, int P) { return C >= 1 && C <= CP_MAX_C && P >= 1 && P <= CP_MAX_P; }
static inline long cp_tiles(long T) { return (T + CP_TOK - 1) / CP_TOK; }
static inline int cp_chunks(long T) { const long n = cp_tiles(T); return (int)(n > CP_MAX_CHUNKS ? CP_MAX_CHUNKS : n); }
// 128 output columns per workgroup where the backward's LDS (weights, tokens, masked gradient) stays below 64 KiB
static inline int cp_pt(int C, int P) { return (P <= 64 || C > 32) ? 64 : 128; }

extern "C" int t4r_cont_proj_supported(int C, int P) { return cp_dims_ok(C, P) ? 1 : 0; }

extern "C" long t4r_cont_proj_bwd_ws_floats(long ntok, int C, int P) {
    if (!cp_dims_ok(C, P) || ntok <= 0 || ntok > INT_MAX) return 0;
    return (long)cp_chunks(ntok) * P * (C + 1);
}

namespace {

struct CPArgs {
    const float* x[CP_MAX_C];
    unsigned long long per_session;     // bit c: column c is [B], one value per session
    const float* W; const float* b;     // [P][C], [P]
    long T; int L, C, P;
    float* out;                         // forward: [T][P]
    const float* dout; long ld; int col;
    float* dpre;                        // backward: [T][P] or null
    float* part;                        // backward: [chunks][P][C + 1]
    float* dW; float* db;
    int chunks;
    int vec_out, vec_g;                 // 16-byte accesses allowed on out / dpre, on dout
};

// W rows p_base .. p_base + PT - 1 transposed into wT[c][PT]; rows beyond P are zero
template <int PT>
__device__ __forceinline__ void cp_stage_w(const CPArgs& a, int p_base, float* wT) {
    const int n = PT * a.C;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int pl = i / a.C, c = i - pl * a.C;
        const int p = p_base + pl;
        wT[c * PT + pl] = p < a.P ? a.W[(long)p * a.C + c] : 0.f;
    }
}

// the C columns' values of tokens t0 .. t0 + 63 into xs[c][64]; tokens beyond T are zero
__device__ __forceinline__ void cp_stage_x(const CPArgs& a, long t0, float* xs) {
    const int n = a.C * CP_TOK;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int c = __builtin_amdgcn_readfirstlane(i >> 6), tl = i & 63;      // a wave's 64 lanes share the column
        const long t = t0 + tl;
        float v = 0.f;
        if (t < a.T) v = a.x[c][(a.per_session >> c) & 1ull ? (long)((int)t / a.L) : t];
        xs[i] = v;
    }
}

// The pre-activations of R consecutive tokens (tile rows r0 ..) x 4 consecutive outputs (tile columns 4 q ..): the one place
// the chain is written, used by the forward and by the backward's mask.
template <int PT, int R>
__device__ __forceinline__ void cp_pre(const float* wT, const float* xs, int C, int q, int r0, const float4 bias, float4 (&acc)[R]) {
#pragma unroll
    for (int i = 0; i < R; ++i) acc[i] = bias;
    for (int c = 0; c < C; ++c) {
        const float4 w = *reinterpret_cast<const float4*>(wT + c * PT + 4 * q);
        float x[R];
#pragma unroll
        for (int i = 0; i < R; i += 4) {
            const float4 v = *reinterpret_cast<const float4*>(xs + c * CP_TOK + r0 + i);
            x[i] = v.x; x[i + 1] = v.y; x[i + 2] = v.z; x[i + 3] = v.w;
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
            acc[i].x = fmaf(w.x, x[i], acc[i].x);
            acc[i].y = fmaf(w.y, x[i], acc[i].y);
            acc[i].z = fmaf(w.z, x[i], acc[i].z);
            acc[i].w = fmaf(w.w, x[i], acc[i].w);
        }
    }
}

__device__ __forceinline__ float4 cp_bias4(const CPArgs& a, int p0) {
    float4 b;
    b.x = p0 < a.P ? a.b[p0] : 0.f;
    b.y = p0 + 1 < a.P ? a.b[p0 + 1] : 0.f;
    b.z = p0 + 2 < a.P ? a.b[p0 + 2] : 0.f;
    b.w = p0 + 3 < a.P ? a.b[p0 + 3] : 0.f;
    return b;
}

// four consecutive values of a dense [T][P] row at column p0 (those below P)
__device__ __forceinline__ void cp_store4(float* row, int p0, int P, bool vec, const float4 v) {
    if (vec && p0 + 3 < P) {
        *reinterpret_cast<float4*>(row + p0) = v;
    } else {
        if (p0 < P) row[p0] = v.x;
        if (p0 + 1 < P) row[p0 + 1] = v.y;
        if (p0 + 2 < P) row[p0 + 2] = v.z;
        if (p0 + 3 < P) row[p0 + 3] = v.w;
    }
}

// ------------------------------------------------------------------------------------------------ forward
// grid (token workgroups, output tiles): workgroup x takes token tiles x, x + gridDim.x, ...
template <int PT>
__global__ __launch_bounds__(256) void cp_fwd_kernel(CPArgs a) {
    constexpr int R = PT / 16, Q = PT / 4;
    extern __shared__ float cp_smem[];
    float* wT = cp_smem;                    // [C][PT]
    float* xs = cp_smem + a.C * PT;         // [C][64]
    const int p_base = blockIdx.y * PT;
    const int q = threadIdx.x % Q, r0 = (threadIdx.x / Q) * R;
    const int p0 = p_base + 4 * q;
    cp_stage_w<PT>(a, p_base, wT);
    const float4 bias = cp_bias4(a, p0);
    const long ntile = (a.T + CP_TOK - 1) / CP_TOK;
    for (long tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const long t0 = tile * CP_TOK;
        if (tile != blockIdx.x) __syncthreads();        // the previous tile's readers are done
        cp_stage_x(a, t0, xs);
        __syncthreads();                                // (the first time: wT is complete too)
        float4 acc[R];
        cp_pre<PT, R>(wT, xs, a.C, q, r0, bias, acc);
        if (p0 >= a.P) continue;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const long t = t0 + r0 + i;
            if (t >= a.T) break;
            const float4 y = make_float4(fmaxf(acc[i].x, 0.f), fmaxf(acc[i].y, 0.f), fmaxf(acc[i].z, 0.f), fmaxf(acc[i].w, 0.f));
            cp_store4(a.out + t * a.P, p0, a.P, a.vec_out != 0, y);
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward
// grid (chunks, output tiles): chunk s takes token tiles s, s + chunks, ...  NC = the columns one thread of the second phase
// accumulates: thread (p = tid % PT, cg = tid / PT) owns columns cg, cg + 256 / PT, ...
template <int PT, int NC>
__global__ __launch_bounds__(256) void cp_bwd_kernel(CPArgs a) {
    constexpr int R = PT / 16, Q = PT / 4, NCG = 256 / PT;
    extern __shared__ float cp_smem[];
    float* wT = cp_smem;                            // [C][PT]
    float* xs = wT + a.C * PT;                      // [C][64]
    float* gs = xs + a.C * CP_TOK;                  // [64][PT]
    const int p_base = blockIdx.y * PT;
    const int q = threadIdx.x % Q, r0 = (threadIdx.x / Q) * R;
    const int p0 = p_base + 4 * q;
    const int pl = threadIdx.x % PT, cg = threadIdx.x / PT;
    cp_stage_w<PT>(a, p_base, wT);
    const float4 bias = cp_bias4(a, p0);
    float dw[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) dw[k] = 0.f;
    float dbias = 0.f;
    const long ntile = (a.T + CP_TOK - 1) / CP_TOK;
    for (long tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const long t0 = tile * CP_TOK;
        // the gradient rows first: their latency runs under the staging of the columns
        float4 gin[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const long t = t0 + r0 + i;
            gin[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < a.T && p0 < a.P) {
                const float* src = a.dout + t * a.ld + a.col + p0;
                if (a.vec_g && p0 + 3 < a.P) {
                    gin[i] = *reinterpret_cast<const float4*>(src);
                } else {
                    gin[i].x = src[0];
                    if (p0 + 1 < a.P) gin[i].y = src[1];
                    if (p0 + 2 < a.P) gin[i].z = src[2];
                    if (p0 + 3 < a.P) gin[i].w = src[3];
                }
            }
        }
        if (tile != blockIdx.x) __syncthreads();        // the previous tile's readers are done
        cp_stage_x(a, t0, xs);
        __syncthreads();                                // (the first time: wT is complete too)
        float4 acc[R];
        cp_pre<PT, R>(wT, xs, a.C, q, r0, bias, acc);
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const long t = t0 + r0 + i;
            float4 g = gin[i];
            if (t < a.T && p0 < a.P) {
                g.x = acc[i].x > 0.f ? g.x : 0.f;
                g.y = acc[i].y > 0.f ? g.y : 0.f;
                g.z = acc[i].z > 0.f ? g.z : 0.f;
                g.w = acc[i].w > 0.f ? g.w : 0.f;
                if (a.dpre) cp_store4(a.dpre + t * a.P, p0, a.P, a.vec_out != 0, g);
            }
            *reinterpret_cast<float4*>(gs + (r0 + i) * PT + 4 * q) = g;
        }
        __syncthreads();
        for (int tl = 0; tl < CP_TOK; tl += 4) {
            const float g0 = gs[tl * PT + pl], g1 = gs[(tl + 1) * PT + pl], g2 = gs[(tl + 2) * PT + pl], g3 = gs[(tl + 3) * PT + pl];
            if (cg == 0) dbias = ((dbias + g0) + g1) + g2 + g3;
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const int c = cg + k * NCG;
                if (c < a.C) {
                    const float4 x = *reinterpret_cast<const float4*>(xs + c * CP_TOK + tl);
                    dw[k] = fmaf(g3, x.w, fmaf(g2, x.z, fmaf(g1, x.y, fmaf(g0, x.x, dw[k]))));
                }
            }
        }
    }
    const int p = p_base + pl;
    if (p < a.P) {
        float* dst = a.part + ((long)blockIdx.x * a.P + p) * (a.C + 1);
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const int c = cg + k * NCG;
            if (c < a.C) dst[c] = dw[k];
        }
        if (cg == 0) dst[a.C] = dbias;
    }
}

// The partials of 16 outputs per workgroup: thread (output o, group sg) adds the chunks of its sixteenth of the chunk range in
// chunk order, thread (o, 0) then the sixteen group sums in group order, then one add into the caller's gradient.  (One
// thread per output walking all the chunks was 256 dependent-latency loads long: most of the backward's time.)
__global__ __launch_bounds__(256) void cp_bwd_finish_kernel(CPArgs a) {
    __shared__ float red[16][16];
    const int o = threadIdx.x & 15, sg = threadIdx.x >> 4;
    const int n = a.P * (a.C + 1);
    const int i = blockIdx.x * 16 + o;
    const int per = (a.chunks + 15) / 16;
    float acc = 0.f;
    if (i < n) {
        const int s1 = min(a.chunks, (sg + 1) * per);
        for (int s = sg * per; s < s1; ++s) acc += a.part[(long)s * n + i];
    }
    red[sg][o] = acc;
    __syncthreads();
    if (sg != 0 || i >= n) return;
    const int p = i / (a.C + 1), c = i - p * (a.C + 1);
    float* dst = c < a.C ? (a.dW ? a.dW + (long)p * a.C + c : nullptr) : (a.db ? a.db + p : nullptr);
    if (!dst) return;
    float t = red[0][o];
#pragma unroll
    for (int g = 1; g < 16; ++g) t += red[g][o];
    *dst += t;
}

}  // namespace

// the sizes both directions share: checked first, and nothing is dereferenced
#define CP_CHECK_DIMS(name)                                                                                                   \
    T4R_CHECK_ARG(C >= 1 && C <= CP_MAX_C, name ": 1 <= C <= 64 continuous columns");                                         \
    T4R_CHECK_ARG(P >= 1 && P <= CP_MAX_P, name ": 1 <= P <= 1024 outputs");                                                  \
    T4R_CHECK_ARG(ntok >= 0 && ntok <= INT_MAX, name ": 0 <= ntok < 2^31");                                                   \
    T4R_CHECK_ARG(L >= 1 && ntok % L == 0, name ": L must be >= 1 and divide ntok");                                          \
    if (ntok == 0) return 0
// the host arrays, read last: fills the kernel's argument block
#define CP_FILL_ARGS(name)                                                                                                    \
    T4R_CHECK_ARG(xs && per_session && W && b, name ": null pointer (xs, per_session, W or b)");                              \
    CPArgs a = {};                                                                                                            \
    for (int c = 0; c < C; ++c) {                                                                                             \
        T4R_CHECK_ARG(xs[c] && (uintptr_t)xs[c] % 4 == 0, name ": a column pointer is null or not 4-byte aligned");           \
        a.x[c] = xs[c];                                                                                                       \
        if (per_session[c]) a.per_session |= 1ull << c;                                                                       \
    }                                                                                                                         \
    a.W = W; a.b = b; a.T = ntok; a.L = L; a.C = C; a.P = P

// one kernel form with `smem` bytes of dynamic LDS (up to 56 KiB) on stream st; the attribute is kept per device
#define CP_LAUNCH(kernel)                                                       \
    do {                                                                        \
        static T4rLdsAttr attr;                                                 \
        t4r_ensure_dynamic_lds((const void*)kernel, smem, attr);                \
        hipLaunchKernelGGL(kernel, grid, dim3(256), smem, st, a);               \
    } while (0)

extern "C" int t4r_cont_proj_fwd(void* stream, const float* const* xs, const int* per_session, long ntok, int L, int C, int P,
                                 const float* W, const float* b, float* out) {
    CP_CHECK_DIMS("cont_proj_fwd");
    T4R_CHECK_ARG(out && (uintptr_t)out % 4 == 0, "cont_proj_fwd: out is null or not 4-byte aligned");
    CP_FILL_ARGS("cont_proj_fwd");
    a.out = out;
    a.vec_out = (P % 4 == 0 && (uintptr_t)out % 16 == 0) ? 1 : 0;
    const int PT = cp_pt(C, P);
    const long ntile = cp_tiles(ntok);
    const dim3 grid((unsigned)(ntile < CP_FWD_WGS ? ntile : CP_FWD_WGS), (unsigned)((P + PT - 1) / PT));
    const size_t smem = (size_t)C * (PT + CP_TOK) * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    if (PT == 64) CP_LAUNCH((cp_fwd_kernel<64>));
    else CP_LAUNCH((cp_fwd_kernel<128>));
    T4R_LAUNCH_CHECK();
    return 0;
}

extern "C" int t4r_cont_proj_bwd(void* stream, const float* dout, long ld, int col, const float* const* xs, const int* per_session,
                                 long ntok, int L, int C, int P, const float* W, const float* b, float* d_w, float* d_b, float* dpre,
                                 float* ws) {
    CP_CHECK_DIMS("cont_proj_bwd");
    T4R_CHECK_ARG(dout && (uintptr_t)dout % 4 == 0 && col >= 0 && ld >= (long)col + P, "cont_proj_bwd: dout null or ld below col + P");
    T4R_CHECK_ARG(ws && (uintptr_t)ws % 4 == 0, "cont_proj_bwd: workspace null or not 4-byte aligned");
    T4R_CHECK_ARG((uintptr_t)d_w % 4 == 0 && (uintptr_t)d_b % 4 == 0 && (uintptr_t)dpre % 4 == 0, "cont_proj_bwd: outputs must be 4-byte aligned");
    CP_FILL_ARGS("cont_proj_bwd");
    a.dout = dout; a.ld = ld; a.col = col; a.dpre = dpre; a.part = ws; a.dW = d_w; a.db = d_b;
    a.chunks = cp_chunks(ntok);
    a.vec_out = (P % 4 == 0 && (uintptr_t)dpre % 16 == 0) ? 1 : 0;
    a.vec_g = (ld % 4 == 0 && col % 4 == 0 && (uintptr_t)dout % 16 == 0) ? 1 : 0;
    const int PT = cp_pt(C, P);
    const dim3 grid((unsigned)a.chunks, (unsigned)((P + PT - 1) / PT));
    const size_t smem = ((size_t)C * (PT + CP_TOK) + (size_t)CP_TOK * PT) * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    if (PT == 64) {
        if (C <= 8) CP_LAUNCH((cp_bwd_kernel<64, 2>));
        else if (C <= 32) CP_LAUNCH((cp_bwd_kernel<64, 8>));
        else CP_LAUNCH((cp_bwd_kernel<64, 16>));
    } else {
        if (C <= 8) CP_LAUNCH((cp_bwd_kernel<128, 4>));
        else CP_LAUNCH((cp_bwd_kernel<128, 16>));
    }
    T4R_LAUNCH_CHECK();
    const int n = P * (C + 1);
    hipLaunchKernelGGL(cp_bwd_finish_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, st, a);
    T4R_LAUNCH_CHECK();
    return 0;
}
