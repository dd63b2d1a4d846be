// XLNet relative-position attention core for attn_type = "uni" (causal), forward and backward (gfx950): include/t4r_hip_uni.h.
//
// HF modeling_xlnet.py with attn_type "uni": create_mask :895-925 puts -1e30 on every key j > i, and relative_positional_encoding
// :940-976 keeps the positions L .. 0 -- the first L + 1 rows of the "bi" encoding; after rel_shift_bnij :81-93 a live pair
// (j <= i) meets row m = j - i + L in [1, L], the index the bi kernels use.  So this is the bi core (xlnet_attn_long.hip) with the
// dead set extended by j > i: same arithmetic, same layout (q, k, v [B L, D], k_r [2 L, D] shared or per session), same dropout
// keys (mask index ((b n_head + h) L + i) L + j), same opt-in key mask (j >= key_len[b] && j != i, unclamped).  What the
// causality buys is used: the loops run over j <= i (i >= j in the key pass), only rows 1 .. L of k_r are read, rows 0 and
// L + 1 .. 2 L - 1 of d k_r are written as exact zeros.
//
// The general form: one thread per query row / key / relative position, blocks of 64 walked by one wave per (session, head), no
// LDS, any L and d_head up to 256 (16-byte requests when the width is a multiple of 4).  The loop bounds are wave-uniform (the
// last row / first key of the block), the pair's own bound is a select, so the rows of the other operand stay broadcast loads.
//   forward          thread = query row i: one online-softmax pass over the keys j <= i; saves the row log-sum-exp
//   backward, rows   thread = query row i: delta_i = d out_i . out_i, dS_ij = scale P_ij (mask_ij d out_i . v_j - delta_i),
//                    d q_i = sum_{j <= i} dS_ij (k_j + k_r[L + j - i]); the two halves summed are d r_w_bias / d r_r_bias
//   backward, keys   thread = key j: d k_j = sum_{i >= j} dS_ij (q_i + r_w_bias), d v_j = sum_{i >= j} P~_ij d out_i; delta_i is
//                    recomputed from the wave-uniform rows of d out and out (no buffer beyond the partial rows)
//   backward, rel    thread = relative position m in [1, L]: d k_r[m] = sum_{i >= L - m} dS_{i, m - L + i} (q_i + r_r_bias)
// Batch-reduced gradients go through the partial buffer and reduction launch of the bi kernels: deterministic.
//
// The LDS-staged form (template parameter LDS; L <= 64 and the tiles within 64 KB: uni_lds_ok): the same kernels, same loops and
// same order of every sum, with the ONE operand that each lane reads at a row of its own taken from LDS instead of memory --
// rows 1 .. L of the head's k_r in the forward, row and key passes (row j - i + L differs lane by lane), the head's k and v rows
// in the relative pass (key m - L + i differs lane by lane).  Those gathers touch up to 64 cache lines per 16-byte request;
// everything wave-uniform stays a broadcast load.  Measured 1.43 x on the core at (B, L, d_head) = (1024, 20, 32); what is left
// is register pressure (one wave per SIMD at d_head 32: DESIGN.md section 4.13).  LDS rows are 16-byte groups, zero-filled past
// d_head (so a width that is not a multiple of 4 reads 16 bytes at a time there too), pitch round_up(d_head, 4) + 4 floats.
#include "t4r_internal.h"
#include "../../include/t4r_hip_uni.h"
#include <stdio.h>
#include <stdlib.h>

#define T4R_KEY_MASKED (-1e30f)

namespace {

// four consecutive floats of a head's row: one 16-byte request when the head width is a multiple of 4, else element by element
// with the row's tail (left elements) zero-filled
__device__ __forceinline__ float4 ld4g(const float* __restrict__ p, int left, bool v4) {
    if (v4) return *reinterpret_cast<const float4*>(p);
    return make_float4(p[0], left > 1 ? p[1] : 0.f, left > 2 ? p[2] : 0.f, left > 3 ? p[3] : 0.f);
}
__device__ __forceinline__ void st4g(float* __restrict__ p, float4 v, int left, bool v4) {
    if (v4) { *reinterpret_cast<float4*>(p) = v; return; }
    p[0] = v.x;
    if (left > 1) p[1] = v.y;
    if (left > 2) p[2] = v.z;
    if (left > 3) p[3] = v.w;
}
// DH is the CAPACITY of the per-thread vectors (registers: every index is a compile-time constant); dh <= DH is the head width
template <int DH>
__device__ __forceinline__ void load_row(float (&x)[DH], const float* __restrict__ p, int dh, bool v4) {
#pragma unroll
    for (int d = 0; d < DH; d += 4) {
        if (d < dh) {
            const float4 t = ld4g(p + d, dh - d, v4);
            x[d] = t.x; x[d + 1] = t.y; x[d + 2] = t.z; x[d + 3] = t.w;
        } else {
            x[d] = 0.f; x[d + 1] = 0.f; x[d + 2] = 0.f; x[d + 3] = 0.f;
        }
    }
}
template <int DH>
__device__ __forceinline__ void store_row(float* __restrict__ p, const float (&x)[DH], int dh, bool v4) {
#pragma unroll
    for (int d = 0; d < DH; d += 4)
        if (d < dh) st4g(p + d, make_float4(x[d], x[d + 1], x[d + 2], x[d + 3]), dh - d, v4);
}
template <int DH>
__device__ __forceinline__ float dot_row(const float (&a)[DH], const float* __restrict__ p, int dh, bool v4) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < DH; d += 4) {
        if (d < dh) {
            const float4 t = ld4g(p + d, dh - d, v4);
            s += a[d] * t.x + a[d + 1] * t.y + a[d + 2] * t.z + a[d + 3] * t.w;
        }
    }
    return s;
}
// a . b of two rows in memory
__device__ __forceinline__ float dot_mem(const float* __restrict__ a, const float* __restrict__ b, int dh, bool v4) {
    float s = 0.f;
    for (int d = 0; d < dh; d += 4) {
        const float4 x = ld4g(a + d, dh - d, v4), y = ld4g(b + d, dh - d, v4);
        s += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
    }
    return s;
}
// (a + bias) . x
template <int DH>
__device__ __forceinline__ float dot_row_bias(const float* __restrict__ a, const float* __restrict__ bias, const float (&x)[DH], int dh, bool v4) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < DH; d += 4) {
        if (d < dh) {
            const float4 t = ld4g(a + d, dh - d, v4);
            const float4 u = ld4g(bias + d, dh - d, v4);
            s += (t.x + u.x) * x[d] + (t.y + u.y) * x[d + 1] + (t.z + u.z) * x[d + 2] + (t.w + u.w) * x[d + 3];
        }
    }
    return s;
}
template <int DH>
__device__ __forceinline__ void axpy_row(float (&acc)[DH], float a, const float* __restrict__ p, int dh, bool v4) {
#pragma unroll
    for (int d = 0; d < DH; d += 4) {
        if (d < dh) {
            const float4 t = ld4g(p + d, dh - d, v4);
            acc[d] += a * t.x; acc[d + 1] += a * t.y; acc[d + 2] += a * t.z; acc[d + 3] += a * t.w;
        }
    }
}
template <int DH>
__device__ __forceinline__ void axpy_row_bias(float (&acc)[DH], float a, const float* __restrict__ p, const float* __restrict__ bias, int dh, bool v4) {
#pragma unroll
    for (int d = 0; d < DH; d += 4) {
        if (d < dh) {
            const float4 t = ld4g(p + d, dh - d, v4);
            const float4 u = ld4g(bias + d, dh - d, v4);
            acc[d] += a * (t.x + u.x); acc[d + 1] += a * (t.y + u.y); acc[d + 2] += a * (t.z + u.z); acc[d + 3] += a * (t.w + u.w);
        }
    }
}

struct UniArgs {
    const float *q, *k, *v, *kr, *rw, *rr;     // [B L, D] x 3; k_r [2 L, D] (+ b kr_bstride); biases [D]
    const float *out, *lse, *dout;             // backward: forward output, row log-sum-exp [B, n, L], upstream gradient
    float *o, *lse_o;                          // forward outputs
    float *dq, *dk, *dv, *dkr_b, *part;
    int B, L, n_head, dh;
    float scale;
    long kr_bstride;
    DropCfg drop;
    const int* key_len;
};

// the opt-in padding rule of the bi kernels; the causal rule (j > i) is the loop bound and a select beside it
#define T4R_PAD_MASKED(j, i, klen) ((j) >= (klen) && (j) != (i))

// LDS-staged form: pitch of a staged row, and the copy of `rows` rows of a head (dh floats at src + r src_pitch) into
// dst[r][pitch] as 16-byte groups, the tail of the last group zero-filled; all 64 lanes take part, barriers are the caller's
__host__ __device__ __forceinline__ int uni_pitch(int dh) { return ((dh + 3) & ~3) + 4; }
__device__ __forceinline__ void stage_rows(float* __restrict__ dst, int pitch, const float* __restrict__ src, long src_pitch,
                                           int rows, int dh, bool v4, int lane) {
    const int g4 = (dh + 3) >> 2;
    for (int e = lane; e < rows * g4; e += 64) {
        const int r = e / g4, c = (e - r * g4) * 4;
        *reinterpret_cast<float4*>(dst + r * pitch + c) = ld4g(src + (long)r * src_pitch + c, dh - c, v4);
    }
}

template <int DH, bool LDS>
__global__ __launch_bounds__(64) void attn_uni_fwd_kernel(UniArgs a) {
    extern __shared__ float4 t4r_uni_smem[];
    float* const skr = reinterpret_cast<float*>(t4r_uni_smem);       // LDS: rows 1 .. L of the head's k_r, [L][pitch]
    const int L = a.L, dh = a.dh, D = a.n_head * dh, h = blockIdx.y, hc = h * dh, lane = threadIdx.x;
    const bool v4 = (dh & 3) == 0, kv4 = LDS || v4;
    const int pitch = uni_pitch(dh);
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const float* krb = a.kr + (long)b * a.kr_bstride + hc;
        const int klen = a.key_len ? a.key_len[b] : L;
        if (LDS && (b == (int)blockIdx.x || a.kr_bstride != 0)) {    // the shared k_r once, a per-session k_r per session
            __syncthreads();
            stage_rows(skr, pitch, krb + D, D, L, dh, v4, lane);
            __syncthreads();
        }
        for (int i0 = 0; i0 < L; i0 += 64) {
            const int i = i0 + lane, ic = min(i, L - 1);
            float qw[DH], qr[DH], o[DH];
            {
                const float* qrow = a.q + ((long)b * L + ic) * D + hc;
#pragma unroll
                for (int d = 0; d < DH; ++d) {
                    const int dc = d < dh ? d : 0;
                    const float t = qrow[dc];
                    qw[d] = d < dh ? t + a.rw[hc + dc] : 0.f; qr[d] = d < dh ? t + a.rr[hc + dc] : 0.f; o[d] = 0.f;
                }
            }
            float m = -INFINITY, l = 0.f;
            const int jmax = min(i0 + 64, L);                // the block's last row sees keys below this; key 0 is live in every row
            for (int j = 0; j < jmax; ++j) {
                const bool on = j <= ic;
                const int jr = on ? j : ic;                   // a dead pair reads the diagonal's row of k_r (rows 1 .. L only)
                const float* krm = LDS ? skr + (jr + L - ic - 1) * pitch : krb + (long)(jr + L - ic) * D;
                float s = dot_row<DH>(qw, a.k + ((long)b * L + j) * D + hc, dh, v4) + dot_row<DH>(qr, krm, dh, kv4);
                s *= a.scale;
                if (T4R_PAD_MASKED(j, ic, klen)) s = T4R_KEY_MASKED;
                const float mn = on ? fmaxf(m, s) : m;
                const float alpha = __expf(m - mn), pj = on ? __expf(s - mn) : 0.f;
                l = l * alpha + pj;
                float pd = pj;
                if (a.drop.p > 0.f) pd *= drop_scale(a.drop, ((unsigned long long)(b * a.n_head + h) * L + ic) * L + j);
#pragma unroll
                for (int d = 0; d < DH; ++d) o[d] *= alpha;
                axpy_row<DH>(o, pd, a.v + ((long)b * L + j) * D + hc, dh, v4);
                m = mn;
            }
            if (i < L) {
                const float inv = 1.f / l;
#pragma unroll
                for (int d = 0; d < DH; ++d) o[d] *= inv;
                store_row<DH>(a.o + ((long)b * L + i) * D + hc, o, dh, v4);
                a.lse_o[((long)b * a.n_head + h) * L + i] = m + __logf(l);
            }
        }
    }
}

template <int DH, bool LDS>
__global__ __launch_bounds__(64) void attn_uni_bwd_rows_kernel(UniArgs a) {
    extern __shared__ float4 t4r_uni_smem[];
    float* const skr = reinterpret_cast<float*>(t4r_uni_smem);       // LDS: rows 1 .. L of the head's k_r, [L][pitch]
    const int L = a.L, dh = a.dh, D = a.n_head * dh, h = blockIdx.y, hc = h * dh, lane = threadIdx.x;
    const bool v4 = (dh & 3) == 0, kv4 = LDS || v4;
    const int pitch = uni_pitch(dh);
    float srw[DH], srr[DH];                     // this lane's share of d r_w_bias / d r_r_bias (all its rows and sessions)
#pragma unroll
    for (int d = 0; d < DH; ++d) { srw[d] = 0.f; srr[d] = 0.f; }
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const float* krb = a.kr + (long)b * a.kr_bstride + hc;
        const int klen = a.key_len ? a.key_len[b] : L;
        if (LDS && (b == (int)blockIdx.x || a.kr_bstride != 0)) {
            __syncthreads();
            stage_rows(skr, pitch, krb + D, D, L, dh, v4, lane);
            __syncthreads();
        }
        for (int i0 = 0; i0 < L; i0 += 64) {
            const int i = i0 + lane, ic = min(i, L - 1);
            const bool live = i < L;
            float qw[DH], qr[DH], g[DH], dqa[DH], dqb[DH];
            const long row = ((long)b * L + ic) * D + hc;
            float delta = 0.f;
#pragma unroll
            for (int d = 0; d < DH; ++d) {
                const bool in = d < dh;
                const int dc = in ? d : 0;
                const float t = a.q[row + dc];
                qw[d] = in ? t + a.rw[hc + dc] : 0.f; qr[d] = in ? t + a.rr[hc + dc] : 0.f;
                g[d] = in ? a.dout[row + dc] : 0.f;
                delta += g[d] * a.out[row + dc];
                dqa[d] = 0.f; dqb[d] = 0.f;
            }
            const float lrow = a.lse[((long)b * a.n_head + h) * L + ic];
            const int jmax = min(i0 + 64, L);
            for (int j = 0; j < jmax; ++j) {
                const bool on = j <= ic;
                const int jr = on ? j : ic;
                const float* kj = a.k + ((long)b * L + j) * D + hc;
                const float* krm = LDS ? skr + (jr + L - ic - 1) * pitch : krb + (long)(jr + L - ic) * D;
                float s = (dot_row<DH>(qw, kj, dh, v4) + dot_row<DH>(qr, krm, dh, kv4)) * a.scale;
                if (T4R_PAD_MASKED(j, ic, klen)) s = T4R_KEY_MASKED;
                const float p = on ? __expf(s - lrow) : 0.f;
                float dp = dot_row<DH>(g, a.v + ((long)b * L + j) * D + hc, dh, v4);
                if (a.drop.p > 0.f) dp *= drop_scale(a.drop, ((unsigned long long)(b * a.n_head + h) * L + ic) * L + j);
                const float ds = on ? p * (dp - delta) * a.scale : 0.f;
                axpy_row<DH>(dqa, ds, kj, dh, v4);
                axpy_row<DH>(dqb, ds, krm, dh, kv4);
            }
            if (live) {
                float* dqrow = a.dq + ((long)b * L + i) * D + hc;
#pragma unroll
                for (int d = 0; d < DH; d += 4)
                    if (d < dh) st4g(dqrow + d, make_float4(dqa[d] + dqb[d], dqa[d + 1] + dqb[d + 1], dqa[d + 2] + dqb[d + 2], dqa[d + 3] + dqb[d + 3]), dh - d, v4);
#pragma unroll
                for (int d = 0; d < DH; ++d) { srw[d] += dqa[d]; srr[d] += dqb[d]; }
            }
        }
    }
    // the workgroup's (= the wave's) sums over its lanes, lane order fixed by the butterfly
    float* mypart = a.part + (long)blockIdx.x * (2L * L * D + 2 * D) + 2L * L * D;
#pragma unroll
    for (int d = 0; d < DH; ++d) {
        float x = srw[d], y = srr[d];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { x += __shfl_xor(x, o, 64); y += __shfl_xor(y, o, 64); }
        if (lane == 0 && d < dh) { mypart[hc + d] = x; mypart[D + hc + d] = y; }
    }
}

template <int DH, bool LDS>
__global__ __launch_bounds__(64) void attn_uni_bwd_keys_kernel(UniArgs a) {
    extern __shared__ float4 t4r_uni_smem[];
    float* const skr = reinterpret_cast<float*>(t4r_uni_smem);       // LDS: rows 1 .. L of the head's k_r, [L][pitch]
    const int L = a.L, dh = a.dh, D = a.n_head * dh, h = blockIdx.y, hc = h * dh, lane = threadIdx.x;
    const bool v4 = (dh & 3) == 0, kv4 = LDS || v4;
    const int pitch = uni_pitch(dh);
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const float* krb = a.kr + (long)b * a.kr_bstride + hc;
        const int klen = a.key_len ? a.key_len[b] : L;
        if (LDS && (b == (int)blockIdx.x || a.kr_bstride != 0)) {
            __syncthreads();
            stage_rows(skr, pitch, krb + D, D, L, dh, v4, lane);
            __syncthreads();
        }
        for (int j0 = 0; j0 < L; j0 += 64) {
            const int j = j0 + lane, jc = min(j, L - 1);
            float kj[DH], vj[DH], dk[DH], dv[DH];
            const long row = ((long)b * L + jc) * D + hc;
            load_row<DH>(kj, a.k + row, dh, v4);
            load_row<DH>(vj, a.v + row, dh, v4);
#pragma unroll
            for (int d = 0; d < DH; ++d) { dk[d] = 0.f; dv[d] = 0.f; }
            for (int i = j0; i < L; ++i) {                                   // the block's first key is seen from row j0 on
                const bool on = jc <= i;
                const float* qi = a.q + ((long)b * L + i) * D + hc;          // wave-uniform rows
                const float* gi = a.dout + ((long)b * L + i) * D + hc;
                const float delta = dot_mem(gi, a.out + ((long)b * L + i) * D + hc, dh, v4);
                float krm[DH];
                const int mrow = on ? jc + L - i : L;
                load_row<DH>(krm, LDS ? skr + (mrow - 1) * pitch : krb + (long)mrow * D, dh, kv4);
                float s = (dot_row_bias<DH>(qi, a.rw + hc, kj, dh, v4) + dot_row_bias<DH>(qi, a.rr + hc, krm, dh, v4)) * a.scale;
                if (T4R_PAD_MASKED(jc, i, klen)) s = T4R_KEY_MASKED;
                const float p = on ? __expf(s - a.lse[((long)b * a.n_head + h) * L + i]) : 0.f;
                float ms = 1.f;
                if (a.drop.p > 0.f) ms = drop_scale(a.drop, ((unsigned long long)(b * a.n_head + h) * L + i) * L + jc);
                const float dp = dot_row<DH>(vj, gi, dh, v4) * ms;
                const float ds = on ? p * (dp - delta) * a.scale : 0.f;
                axpy_row_bias<DH>(dk, ds, qi, a.rw + hc, dh, v4);
                axpy_row<DH>(dv, p * ms, gi, dh, v4);
            }
            if (j < L) {
                store_row<DH>(a.dk + row, dk, dh, v4);
                store_row<DH>(a.dv + row, dv, dh, v4);
            }
        }
    }
}

template <int DH, bool SHARED_KR, bool LDS>
__global__ __launch_bounds__(64) void attn_uni_bwd_rel_kernel(UniArgs a) {
    extern __shared__ float4 t4r_uni_smem[];
    const int L = a.L, dh = a.dh, D = a.n_head * dh, h = blockIdx.y, hc = h * dh, lane = threadIdx.x;
    const bool v4 = (dh & 3) == 0, kv4 = LDS || v4;
    const int pitch = uni_pitch(dh);
    float* const sk = reinterpret_cast<float*>(t4r_uni_smem);        // LDS: the (session, head)'s k and v rows, 2 x [L][pitch]
    float* const sv = sk + L * pitch;
    for (int m0 = 0; m0 < 2 * L; m0 += 64) {
        const int m = m0 + lane;
        const bool used = m >= 1 && m <= L;             // rows 0 and L + 1 .. 2 L - 1 meet no live pair: exact zeros
        const int mc = min(max(m, 1), L);
        const int ilo = max(0, L - min(m0 + 63, L));    // the block's largest position meets key 0 at this row
        float acc[DH];
#pragma unroll
        for (int d = 0; d < DH; ++d) acc[d] = 0.f;
        for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
            if (!SHARED_KR) {
#pragma unroll
                for (int d = 0; d < DH; ++d) acc[d] = 0.f;
            }
            if (m0 <= L) {                              // (wave-uniform) a block of positions above L has nothing to sum
                const float* krb = a.kr + (long)b * a.kr_bstride + hc;
                const int klen = a.key_len ? a.key_len[b] : L;
                float krm[DH];
                load_row<DH>(krm, krb + (long)mc * D, dh, v4);
                if (LDS) {
                    __syncthreads();
                    stage_rows(sk, pitch, a.k + (long)b * L * D + hc, D, L, dh, v4, lane);
                    stage_rows(sv, pitch, a.v + (long)b * L * D + hc, D, L, dh, v4, lane);
                    __syncthreads();
                }
                for (int i = ilo; i < L; ++i) {
                    const int j = mc - L + i;                       // the key this relative position meets query i at (<= i)
                    const bool hit = used && j >= 0;
                    const int jc = max(j, 0);
                    const float* qi = a.q + ((long)b * L + i) * D + hc;
                    const float* gi = a.dout + ((long)b * L + i) * D + hc;
                    const float delta = dot_mem(gi, a.out + ((long)b * L + i) * D + hc, dh, v4);
                    float kj[DH];
                    load_row<DH>(kj, LDS ? sk + jc * pitch : a.k + ((long)b * L + jc) * D + hc, dh, kv4);
                    float s = (dot_row_bias<DH>(qi, a.rw + hc, kj, dh, v4) + dot_row_bias<DH>(qi, a.rr + hc, krm, dh, v4)) * a.scale;
                    if (T4R_PAD_MASKED(jc, i, klen)) s = T4R_KEY_MASKED;
                    const float p = hit ? __expf(s - a.lse[((long)b * a.n_head + h) * L + i]) : 0.f;
                    float dp;
                    {
                        float vj[DH];
                        load_row<DH>(vj, LDS ? sv + jc * pitch : a.v + ((long)b * L + jc) * D + hc, dh, kv4);
                        dp = dot_row<DH>(vj, gi, dh, v4);
                    }
                    if (a.drop.p > 0.f) dp *= drop_scale(a.drop, ((unsigned long long)(b * a.n_head + h) * L + i) * L + jc);
                    const float ds = hit ? p * (dp - delta) * a.scale : 0.f;
                    axpy_row_bias<DH>(acc, ds, qi, a.rr + hc, dh, v4);
                }
            }
            if (!SHARED_KR && m < 2 * L) {
                if (!used) {
#pragma unroll
                    for (int d = 0; d < DH; ++d) acc[d] = 0.f;
                }
                store_row<DH>(a.dkr_b + ((long)b * 2 * L + m) * D + hc, acc, dh, v4);
            }
        }
        if (SHARED_KR && m < 2 * L) {
            if (!used) {
#pragma unroll
                for (int d = 0; d < DH; ++d) acc[d] = 0.f;
            }
            store_row<DH>(a.part + (long)blockIdx.x * (2L * L * D + 2 * D) + (long)m * D + hc, acc, dh, v4);
        }
    }
}

// capacity of the per-thread vectors for a head width
int cap_of(int d_head) { return d_head <= 8 ? 8 : d_head <= 16 ? 16 : d_head <= 32 ? 32 : d_head <= 64 ? 64 : d_head <= 128 ? 128 : 256; }

// the LDS-staged form takes the shape: one row block, and the larger of the two tilings (k and v rows of the relative pass)
// within the 64 KB a launch may ask for without an attribute
bool uni_lds_ok(int L, int d_head) { return L <= 64 && 2L * L * uni_pitch(d_head) * (long)sizeof(float) <= 64 * 1024; }

int args_ok(const char* who, int L, int n_head, int d_head) {
    if (L >= 1 && n_head >= 1 && d_head >= 1 && d_head <= 256) return 0;
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: needs L >= 1, n_head >= 1 and d_head in [1, 256]", who);
    t4r_set_error(msg);
    return -1;
}

}  // namespace

extern "C" int t4r_xlnet_attn_uni_fwd(void* stream, const float* q, const float* k, const float* v, const float* k_r,
                                      const float* r_w_bias, const float* r_r_bias, float* out, float* lse, int B, int L,
                                      int n_head, int d_head, int kr_per_batch, float drop_p, unsigned long long seed,
                                      unsigned long long ctr_hi, const int* key_len) {
    if (B == 0) return 0;
    if (args_ok("xlnet_attn_uni", L, n_head, d_head)) return -1;
    T4R_CHECK_ARG(q && k && v && k_r && r_w_bias && r_r_bias && out && lse, "xlnet_attn_uni: null pointer");
    hipStream_t st = (hipStream_t)stream;
    UniArgs a{};
    a.q = q; a.k = k; a.v = v; a.kr = k_r; a.rw = r_w_bias; a.rr = r_r_bias; a.o = out; a.lse_o = lse;
    a.B = B; a.L = L; a.n_head = n_head; a.dh = d_head; a.scale = 1.0f / sqrtf((float)d_head);
    a.kr_bstride = kr_per_batch ? 2L * L * n_head * d_head : 0; a.drop = make_drop(drop_p, seed, ctr_hi); a.key_len = key_len;
    const dim3 grid(B < 8192 ? B : 8192, n_head), block(64);
    const bool lds = uni_lds_ok(L, d_head);
    const size_t sm1 = lds ? (size_t)L * uni_pitch(d_head) * sizeof(float) : 0;       // rows 1 .. L of the head's k_r
#define T4R_UNI_FWD(DHV)                                                                              \
    if (lds) hipLaunchKernelGGL((attn_uni_fwd_kernel<DHV, true>), grid, block, sm1, st, a);           \
    else hipLaunchKernelGGL((attn_uni_fwd_kernel<DHV, false>), grid, block, 0, st, a);
    switch (cap_of(d_head)) {
        case 8: T4R_UNI_FWD(8) break;
        case 16: T4R_UNI_FWD(16) break;
        case 32: T4R_UNI_FWD(32) break;
        case 64: T4R_UNI_FWD(64) break;
        case 128: T4R_UNI_FWD(128) break;
        default: T4R_UNI_FWD(256) break;
    }
#undef T4R_UNI_FWD
    T4R_LAUNCH_CHECK();
    return 0;
}

// the workspace holds one partial row (2 L D + 2 D floats) per workgroup of t4r_xlnet_attn_bwd_blocks(B): the head of what
// t4r_xlnet_attn_bwd_ws_floats sizes for every shape
int t4r_xlnet_attn_uni_bwd_impl(void* stream, const float* q, const float* k, const float* v, const float* k_r,
                                const float* r_w_bias, const float* r_r_bias, const float* out, const float* lse,
                                const float* dout, float* dq, float* dk, float* dv, float* dk_r, float* d_r_w_bias,
                                float* d_r_r_bias, float* workspace, int B, int L, int n_head, int d_head, int kr_per_batch,
                                float drop_p, unsigned long long seed, unsigned long long ctr_hi, const int* key_len,
                                ReduceCtx* red) {
    if (B == 0) return 0;
    if (args_ok("xlnet_attn_uni_bwd", L, n_head, d_head)) return -1;
    T4R_CHECK_ARG(q && k && v && k_r && r_w_bias && r_r_bias && out && lse && dout && dq && dk && dv && dk_r && d_r_w_bias &&
                  d_r_r_bias && workspace, "xlnet_attn_uni_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int D = n_head * d_head, nblocks = t4r_xlnet_attn_bwd_blocks(B);
    const bool shared = !kr_per_batch;
    UniArgs a{};
    a.q = q; a.k = k; a.v = v; a.kr = k_r; a.rw = r_w_bias; a.rr = r_r_bias; a.out = out; a.lse = lse; a.dout = dout;
    a.dq = dq; a.dk = dk; a.dv = dv; a.part = workspace; a.dkr_b = shared ? nullptr : dk_r;
    a.B = B; a.L = L; a.n_head = n_head; a.dh = d_head; a.scale = 1.0f / sqrtf((float)d_head);
    a.kr_bstride = shared ? 0 : 2L * L * D; a.drop = make_drop(drop_p, seed, ctr_hi); a.key_len = key_len;
    const dim3 grid(nblocks, n_head), block(64);
    const bool lds = uni_lds_ok(L, d_head);
    const size_t sm1 = lds ? (size_t)L * uni_pitch(d_head) * sizeof(float) : 0;       // k_r rows (row and key passes)
    const size_t sm2 = 2 * sm1;                                                       // k and v rows (relative pass)
#define T4R_UNI_BWD_L(DHV, LDSV)                                                                                 \
    hipLaunchKernelGGL((attn_uni_bwd_rows_kernel<DHV, LDSV>), grid, block, sm1, st, a);                          \
    hipLaunchKernelGGL((attn_uni_bwd_keys_kernel<DHV, LDSV>), grid, block, sm1, st, a);                          \
    if (shared) hipLaunchKernelGGL((attn_uni_bwd_rel_kernel<DHV, true, LDSV>), grid, block, sm2, st, a);         \
    else hipLaunchKernelGGL((attn_uni_bwd_rel_kernel<DHV, false, LDSV>), grid, block, sm2, st, a);
#define T4R_UNI_BWD(DHV)                     \
    if (lds) { T4R_UNI_BWD_L(DHV, true) }    \
    else { T4R_UNI_BWD_L(DHV, false) }
    switch (cap_of(d_head)) {
        case 8: T4R_UNI_BWD(8) break;
        case 16: T4R_UNI_BWD(16) break;
        case 32: T4R_UNI_BWD(32) break;
        case 64: T4R_UNI_BWD(64) break;
        case 128: T4R_UNI_BWD(128) break;
        default: T4R_UNI_BWD(256) break;
    }
#undef T4R_UNI_BWD
#undef T4R_UNI_BWD_L
    T4R_LAUNCH_CHECK();
    // d k_r overwritten (shared k_r: summed over the workgroups here), bias gradients accumulated
    return t4r_reduce_partials_launch(st, workspace, nblocks, shared ? dk_r : nullptr, 2 * L * D, 0, d_r_w_bias, D, 1, d_r_r_bias,
                                      D, 1, red);
}

extern "C" int t4r_xlnet_attn_uni_bwd(void* stream, const float* q, const float* k, const float* v, const float* k_r,
                                      const float* r_w_bias, const float* r_r_bias, const float* out, const float* lse,
                                      const float* dout, float* dq, float* dk, float* dv, float* dk_r, float* d_r_w_bias,
                                      float* d_r_r_bias, float* workspace, int B, int L, int n_head, int d_head,
                                      int kr_per_batch, float drop_p, unsigned long long seed, unsigned long long ctr_hi,
                                      const int* key_len) {
    return t4r_xlnet_attn_uni_bwd_impl(stream, q, k, v, k_r, r_w_bias, r_r_bias, out, lse, dout, dq, dk, dv, dk_r, d_r_w_bias,
                                       d_r_r_bias, workspace, B, L, n_head, d_head, kr_per_batch, drop_p, seed, ctr_hi, key_len,
                                       nullptr);
}
