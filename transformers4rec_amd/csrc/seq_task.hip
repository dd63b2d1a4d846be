// Session-level prediction tasks (include/t4r_hip_seqtask.h): summary of the body's output over the sequence (first / last /
// mean), the Linear(D, 1) over it, sigmoid or identity, the row loss (BCE or MSE) and its mean; and the backward of all of it.
// gfx950 only.
//
// Forward, two launches.  (1) one 64-lane wave per session, four waves per workgroup: lane i owns the column quads
// 4 (i + 64 j), j = 0, 1, ... (D <= 1024: at most four), walks the positions in order with one fp32 chain per column, stores
// s_b, and folds w . s_b into one partial per lane (quads ascending, columns ascending); the 64 partials meet in a butterfly
// of cross-lane moves (no LDS), lane 0 applies the bias, the activation and the row loss.  The column-to-lane map is the same
// with 16-byte and with 4-byte loads: the two paths give the same bits.  (2) one workgroup adds the B row losses in a fixed
// order (thread t: rows t, t + 256, ... ascending; then a halving tree) and stores their mean.  Inference stops after (1).
//
// Backward, two launches.  (1) has two kinds of workgroups.  The first B * segs write dx: session b's [L, D] block is one
// contiguous run, cut into segments of 4096 floats, each element coef_b(l) * w[d] or 0 -- a pure streaming write; every
// workgroup derives dz_b from (g, pred_b, target_b) itself.  The remaining `chunks` workgroups each take a run of sessions and
// add dz_b * s_b[d] over them in session order (thread t owns columns t, t + 256, ...), leaving a [D + 1] partial in the
// workspace (the last entry is d b).  (2) adds the partials in chunk order and adds the sum into the caller's gradients.
// No float atomics anywhere; every sum has one fixed order.
#include "t4r_common.h"
#include <limits.h>

#define ST_MAX_L 1023
#define ST_MAX_D 1024
#define ST_CHUNK 32              // sessions per chunk of the parameter-gradient reduction while there are few of them
#define ST_MAX_CHUNKS 256        // ... and the most chunks
#define ST_SEG 4096              // floats of dx per workgroup

static inline bool st_dims_ok(int L, int D) { return L >= 1 && L <= ST_MAX_L && D >= 1 && D <= ST_MAX_D; }
static inline int st_chunks(long B) { const long n = (B + ST_CHUNK - 1) / ST_CHUNK; return (int)(n > ST_MAX_CHUNKS ? ST_MAX_CHUNKS : n); }

extern "C" int t4r_seq_task_supported(int L, int D) { return st_dims_ok(L, D) ? 1 : 0; }

extern "C" long t4r_seq_task_ws_floats(long B, int D) {
    if (B <= 0 || B > INT_MAX || D < 1 || D > ST_MAX_D) return 0;
    return B + (long)st_chunks(B) * (D + 1);
}

namespace {

struct STArgs {
    const float* x; const int* len; const float* w; const float* b; const float* target;
    const float* g; const float* pred_in; const float* s_in;       // backward
    float* s; float* pred; float* loss;                            // forward
    float* dx; float* dW; float* db;                               // backward
    float* ws;                                                     // [B] row losses | dz, then [chunks][D + 1] partials
    long B, per;                                                   // per: sessions per chunk
    int L, D, summary, act, loss_kind, chunks, segs;
    unsigned n_dx;                                                 // workgroups of the backward that write dx
    float invB;
};

__device__ __forceinline__ int st_count(const STArgs& a, long b) {
    if (!a.len) return a.L;
    const int n = a.len[b];
    return n < 0 ? 0 : (n > a.L ? a.L : n);
}

// four consecutive floats at p of which the first `left` exist (VEC: all four, 16-byte aligned)
template <bool VEC>
__device__ __forceinline__ float4 st_load4(const float* p, int left) {
    if (VEC) return *reinterpret_cast<const float4*>(p);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    v.x = p[0];
    if (left > 1) v.y = p[1];
    if (left > 2) v.z = p[2];
    if (left > 3) v.w = p[3];
    return v;
}
template <bool VEC>
__device__ __forceinline__ void st_store4(float* p, int left, const float4 v) {
    if (VEC) { *reinterpret_cast<float4*>(p) = v; return; }
    p[0] = v.x;
    if (left > 1) p[1] = v.y;
    if (left > 2) p[2] = v.z;
    if (left > 3) p[3] = v.w;
}

// ------------------------------------------------------------------------------------------------ forward
template <bool VEC>
__global__ __launch_bounds__(256) void st_fwd_kernel(STArgs a) {
    const int lane = threadIdx.x & 63;
    const long b = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= a.B) return;                   // the whole wave
    const int n = st_count(a, b);
    const float* xb = a.x + b * (long)a.L * a.D;
    float* sb = a.s + b * (long)a.D;
    float part = 0.f;
    for (int c0 = 4 * lane; c0 < a.D; c0 += 256) {
        const int left = a.D - c0;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n > 0) {
            if (a.summary == 2) {
#pragma unroll 4
                for (int l = 0; l < n; ++l) {
                    const float4 v = st_load4<VEC>(xb + (long)l * a.D + c0, left);
                    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
                }
                const float fn = (float)n;
                acc.x /= fn; acc.y /= fn; acc.z /= fn; acc.w /= fn;
            } else {
                acc = st_load4<VEC>(xb + (long)(a.summary == 0 ? 0 : n - 1) * a.D + c0, left);
            }
        }
        st_store4<VEC>(sb + c0, left, acc);
        const float4 w = st_load4<VEC>(a.w + c0, left);        // components beyond D are 0 on both sides
        part = fmaf(w.x, acc.x, part);
        part = fmaf(w.y, acc.y, part);
        part = fmaf(w.z, acc.z, part);
        part = fmaf(w.w, acc.w, part);
    }
    const float dot = wave_sum(part);
    if (lane != 0) return;
    const float z = (a.b ? a.b[0] : 0.f) + dot;
    const float p = a.act ? 1.f / (1.f + expf(-z)) : z;
    a.pred[b] = p;
    if (!a.target) return;
    const float t = a.target[b];
    float row;
    if (a.loss_kind == 0) {
        row = (p - t) * (p - t);
    } else {
        // torch.nn.BCELoss: both logarithms clamped at -100; log1p keeps log(1 - p) accurate where p is small
        row = 0.f - (t * fmaxf(logf(p), -100.f) + (1.f - t) * fmaxf(log1pf(-p), -100.f));
    }
    a.ws[b] = row;
}

__global__ __launch_bounds__(256) void st_loss_kernel(STArgs a) {
    __shared__ float red[256];
    float acc = 0.f;
    for (long i = threadIdx.x; i < a.B; i += 256) acc += a.ws[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.loss[0] = red[0] / (float)a.B;
}

// ------------------------------------------------------------------------------------------------ backward
// d loss / d z_b from the forward's notes: torch's mse_loss_backward / binary_cross_entropy_backward, then sigmoid_backward.
// gs = g * (1 / B) is formed first, so that a session's gradient depends on B through that one factor only.
__device__ __forceinline__ float st_dz(const STArgs& a, float gs, long b) {
    const float p = a.pred_in[b], t = a.target[b];
    const float pq = (1.f - p) * p;
    float d = a.loss_kind == 0 ? gs * (2.f * (p - t)) : gs * (p - t) / fmaxf(pq, 1e-12f);
    if (a.act) d *= pq;
    return d;
}

template <bool VEC>
__global__ __launch_bounds__(256) void st_bwd_kernel(STArgs a) {
    const float gs = a.g[0] * a.invB;
    if (blockIdx.x < a.n_dx) {
        const long b = blockIdx.x / (unsigned)a.segs;
        const int seg = (int)(blockIdx.x - (unsigned)b * (unsigned)a.segs);
        const int n = st_count(a, b);
        const float dz = st_dz(a, gs, b);
        if (seg == 0 && threadIdx.x == 0) a.ws[b] = dz;
        // rows [lo, hi) of the session get coef * w, the others 0
        int lo = 0, hi = 0;
        float coef = dz;
        if (n > 0) {
            if (a.summary == 0) { hi = 1; }
            else if (a.summary == 1) { lo = n - 1; hi = n; }
            else { hi = n; coef = dz / (float)n; }
        }
        const int LD = a.L * a.D;               // <= 1023 * 1024
        float* dxb = a.dx + b * (long)LD;
        const int e0 = seg * ST_SEG;
        const int e1 = e0 + ST_SEG < LD ? e0 + ST_SEG : LD;
        if (VEC) {
            for (int e = e0 + 4 * (int)threadIdx.x; e < e1; e += 1024) {
                const int l = e / a.D, d = e - l * a.D;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (l >= lo && l < hi) {
                    const float4 w = *reinterpret_cast<const float4*>(a.w + d);
                    v = make_float4(coef * w.x, coef * w.y, coef * w.z, coef * w.w);
                }
                *reinterpret_cast<float4*>(dxb + e) = v;
            }
        } else {
            for (int e = e0 + (int)threadIdx.x; e < e1; e += 256) {
                const int l = e / a.D, d = e - l * a.D;
                dxb[e] = (l >= lo && l < hi) ? coef * a.w[d] : 0.f;
            }
        }
        return;
    }
    // parameter gradients of one chunk of sessions
    __shared__ float dzs[256];
    const long c = (long)(blockIdx.x - a.n_dx);
    const long b0 = c * a.per;
    const long b1 = b0 + a.per < a.B ? b0 + a.per : a.B;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    float accb = 0.f;
    for (long bb = b0; bb < b1; bb += 256) {
        const int m = (int)(b1 - bb < 256 ? b1 - bb : 256);
        __syncthreads();
        if ((int)threadIdx.x < m) dzs[threadIdx.x] = st_dz(a, gs, bb + threadIdx.x);
        __syncthreads();
        for (int i = 0; i < m; ++i) {
            const float dz = dzs[i];
            const float* sb = a.s_in + (bb + i) * (long)a.D;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int d = (int)threadIdx.x + 256 * k;
                if (d < a.D) acc[k] = fmaf(dz, sb[d], acc[k]);
            }
            accb += dz;
        }
    }
    float* dst = a.ws + a.B + c * (long)(a.D + 1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = (int)threadIdx.x + 256 * k;
        if (d < a.D) dst[d] = acc[k];
    }
    if (threadIdx.x == 0) dst[a.D] = accb;
}

// 16 outputs per workgroup: thread (output o, group sg) adds its sixteenth of the chunks in chunk order, thread (o, 0) the
// sixteen group sums in group order, then one add into the caller's gradient (the form of cont_proj.hip's finish kernel)
__global__ __launch_bounds__(256) void st_bwd_finish_kernel(STArgs a) {
    __shared__ float red[16][16];
    const int o = threadIdx.x & 15, sg = threadIdx.x >> 4;
    const int n = a.D + 1;
    const int i = blockIdx.x * 16 + o;
    const int per = (a.chunks + 15) / 16;
    const float* part = a.ws + a.B;
    float acc = 0.f;
    if (i < n) {
        const int s1 = min(a.chunks, (sg + 1) * per);
        for (int s = sg * per; s < s1; ++s) acc += part[(long)s * n + i];
    }
    red[sg][o] = acc;
    __syncthreads();
    if (sg != 0 || i >= n) return;
    float* dst = i < a.D ? (a.dW ? a.dW + i : nullptr) : a.db;
    if (!dst) return;
    float t = red[0][o];
#pragma unroll
    for (int k = 1; k < 16; ++k) t += red[k][o];
    *dst += t;
}

}  // namespace

#define ST_ALIGNED4(p) ((uintptr_t)(p) % 4 == 0)
#define ST_ALIGNED16(p) ((uintptr_t)(p) % 16 == 0)
// the sizes and selectors both directions share: checked first, and nothing is dereferenced
#define ST_CHECK_DIMS(name)                                                                                                   \
    T4R_CHECK_ARG(L >= 1 && L <= ST_MAX_L, name ": 1 <= L <= 1023 positions");                                                \
    T4R_CHECK_ARG(D >= 1 && D <= ST_MAX_D, name ": 1 <= D <= 1024 columns");                                                  \
    T4R_CHECK_ARG(B >= 0 && B <= INT_MAX, name ": 0 <= B < 2^31 sessions");                                                   \
    T4R_CHECK_ARG(summary >= 0 && summary <= 2, name ": summary must be 0 (first), 1 (last) or 2 (mean)");                    \
    T4R_CHECK_ARG(act == 0 || act == 1, name ": act must be 0 (identity) or 1 (sigmoid)");                                    \
    T4R_CHECK_ARG(loss_kind == 0 || loss_kind == 1, name ": loss_kind must be 0 (MSE) or 1 (BCE)");                           \
    T4R_CHECK_ARG(!(loss_kind == 1 && act == 0), name ": the BCE loss needs act = 1 (probabilities)");                        \
    if (B == 0) return 0

extern "C" int t4r_seq_task_fwd(void* stream, const float* x, const int* len, long B, int L, int D, int summary, const float* w,
                                const float* b, int act, int loss_kind, const float* target, float* s, float* pred, float* loss,
                                float* ws) {
    ST_CHECK_DIMS("seq_task_fwd");
    T4R_CHECK_ARG(x && w && s && pred, "seq_task_fwd: null pointer (x, w, s or pred)");
    T4R_CHECK_ARG(!target || (loss && ws), "seq_task_fwd: a target needs loss and ws");
    T4R_CHECK_ARG(ST_ALIGNED4(x) && ST_ALIGNED4(len) && ST_ALIGNED4(w) && ST_ALIGNED4(b) && ST_ALIGNED4(target) && ST_ALIGNED4(s)
                      && ST_ALIGNED4(pred) && ST_ALIGNED4(loss) && ST_ALIGNED4(ws),
                  "seq_task_fwd: every pointer must be 4-byte aligned");
    STArgs a = {};
    a.x = x; a.len = len; a.w = w; a.b = b; a.target = target; a.s = s; a.pred = pred; a.loss = loss; a.ws = ws;
    a.B = B; a.L = L; a.D = D; a.summary = summary; a.act = act; a.loss_kind = loss_kind;
    const bool vec = D % 4 == 0 && ST_ALIGNED16(x) && ST_ALIGNED16(w) && ST_ALIGNED16(s);
    const dim3 grid((unsigned)((B + 3) / 4));
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(st_fwd_kernel<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(st_fwd_kernel<false>, grid, dim3(256), 0, st, a);
    T4R_LAUNCH_CHECK();
    if (!target) return 0;
    hipLaunchKernelGGL(st_loss_kernel, dim3(1), dim3(256), 0, st, a);
    T4R_LAUNCH_CHECK();
    return 0;
}

extern "C" int t4r_seq_task_bwd(void* stream, const float* g, const float* pred, const float* target, const float* s, const int* len,
                                long B, int L, int D, int summary, const float* w, int act, int loss_kind, float* dx, float* d_w,
                                float* d_b, float* ws) {
    ST_CHECK_DIMS("seq_task_bwd");
    T4R_CHECK_ARG(g && pred && target && s && w && dx && ws, "seq_task_bwd: null pointer (g, pred, target, s, w, dx or ws)");
    T4R_CHECK_ARG(ST_ALIGNED4(g) && ST_ALIGNED4(pred) && ST_ALIGNED4(target) && ST_ALIGNED4(s) && ST_ALIGNED4(len) && ST_ALIGNED4(w)
                      && ST_ALIGNED4(dx) && ST_ALIGNED4(d_w) && ST_ALIGNED4(d_b) && ST_ALIGNED4(ws),
                  "seq_task_bwd: every pointer must be 4-byte aligned");
    STArgs a = {};
    a.g = g; a.pred_in = pred; a.target = target; a.s_in = s; a.len = len; a.w = w; a.dx = dx; a.dW = d_w; a.db = d_b; a.ws = ws;
    a.B = B; a.L = L; a.D = D; a.summary = summary; a.act = act; a.loss_kind = loss_kind;
    a.invB = 1.f / (float)B;
    a.segs = (L * D + ST_SEG - 1) / ST_SEG;
    const long n_dx = B * a.segs;
    const bool params = d_w || d_b;
    a.chunks = params ? st_chunks(B) : 0;
    a.per = params ? (B + a.chunks - 1) / a.chunks : 0;
    T4R_CHECK_ARG(n_dx + a.chunks <= INT_MAX, "seq_task_bwd: B * ceil(L * D / 4096) must stay below 2^31");
    a.n_dx = (unsigned)n_dx;
    const bool vec = D % 4 == 0 && ST_ALIGNED16(dx) && ST_ALIGNED16(w);
    const dim3 grid((unsigned)(n_dx + a.chunks));
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(st_bwd_kernel<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(st_bwd_kernel<false>, grid, dim3(256), 0, st, a);
    T4R_LAUNCH_CHECK();
    if (!params) return 0;
    hipLaunchKernelGGL(st_bwd_finish_kernel, dim3((unsigned)((D + 1 + 15) / 16)), dim3(256), 0, st, a);
    T4R_LAUNCH_CHECK();
    return 0;
}
