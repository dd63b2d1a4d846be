// Replaced-token-detection head (include/t4r_hip_rtd.h): Linear(D, D) + activation + Linear(D, 1) over every token, the
// BCE-with-logits loss over the active tokens, and the backward of all of it.  gfx950 only.
//
// Tile kernel (forward and backward share it).  A workgroup of four waves owns one chunk of 128 consecutive tokens, a wave
// 32 of them.  W1 goes through LDS in tiles of 64 rows p (pitch D + 4 floats; 64 rows of D = 512 are 129 KB, all of W1 at
// D = 256 would be 256 KB), staged once per workgroup and tile.  Per tile a wave forms a^T = W1 x^T on the fp32 matrix cores
// (v_mfma_f32_32x32x2_f32: bit for bit an fp32 fma chain per element, seeded with b1[p]): two 32 x 32 accumulators with the
// token on the lane and p in the registers (mfma_frag.h's map).  The contraction index d runs d = kh D/2 + s, s ascending,
// kh = 0 before kh = 1 inside a step; x is read straight from global memory as each lane's own row fragment.
//   forward:  h = act(a), one fma chain per lane over its p (tile, accumulator, register ascending) of w2[p] h; the two lane
//             halves meet in one add, z = b2 + (half 0 + half 1).  The row loss goes to ws[t] (0 for an inactive token).
//   backward: the same a (the same instructions on the same operands: the same bits), da = (dz w2[p]) act'(a) in the
//             accumulator's registers.  That register image IS the A operand of dx = da W1 (the contraction runs over the
//             accumulator's row index p), so dx needs no exchange: 16 matrix instructions per accumulator and 32 columns of
//             dx, B operand W1[p][d] from the staged tile.  dx is accumulated over the p tiles through its own memory (tile 0
//             stores, later tiles load, add and store -- the same lane, the same address).  da is also stored to ws [T, D] for
//             the d W1 kernel, and the column sums of da (d b1), dz h (d w2) and dz (d b2) over the chunk's tokens -- a
//             butterfly over the wave's 32 tokens, then the four waves in token order -- go to ws as one partial per chunk.
// d W1 kernel: one wave per 64 x 64 tile of d W1 and per split of the token range; da^T x on the matrix cores, tokens
// ascending; the partial tiles go to ws.  Finish kernels: the forward's adds the T row losses (thread t: rows t, t + 1024, ...
// ascending, then a halving tree), counts the active tokens and stores n and the mean; the backward's adds the d W1 partials
// in split order and the chunk partials in chunk order and ADDS each sum into the caller's gradient.
// No float atomics; every sum has one fixed order; a token's z and dx do not depend on where it sits in the launch.
#include "../../include/t4r_hip_rtd.h"
#include "mfma_frag.h"
#include <limits.h>

#define RH_TOK 128               // tokens per workgroup of the tile kernel (four waves of 32)
#define RH_PT 64                 // rows of W1 per LDS tile (two 32 x 32 accumulators per wave)
#define RH_WSPLIT_FLOATS (4l << 20)   // d W1 partials: at most max(D^2, 4 Mi) floats

static inline bool rh_dim_ok(int D) { return D >= 16 && D <= 512 && D % 16 == 0; }
static inline long rh_chunks(long T) { return (T + RH_TOK - 1) / RH_TOK; }
static inline long rh_part_stride(int D) { return 2l * D + 4; }          // [d b1 | d w2 | d b2, 3 unused]: a multiple of 4
static inline long rh_splits(long T, int D) {
    long s = (T + 63) / 64, cap = RH_WSPLIT_FLOATS / ((long)D * D);
    if (cap < 1) cap = 1;
    return s < cap ? s : cap;
}
static inline long rh_wpart_floats(long T, int D) {
    const long a = ((T + 63) / 64) * D * D, b = (long)D * D > RH_WSPLIT_FLOATS ? (long)D * D : RH_WSPLIT_FLOATS;
    return a < b ? a : b;
}

extern "C" int t4r_rtd_head_supported(int D) { return rh_dim_ok(D) ? 1 : 0; }

extern "C" long t4r_rtd_head_ws_floats(long ntok, int D) {
    if (ntok <= 0 || ntok > INT_MAX || !rh_dim_ok(D)) return 0;
    return ntok * D + rh_chunks(ntok) * rh_part_stride(D) + rh_wpart_floats(ntok, D);
}

namespace {

struct RHArgs {
    const float* x; const unsigned char* active; const unsigned char* label;
    const float* W1; const float* b1; const float* w2; const float* b2;
    const float* g; const float* z_in; const int* n_in;            // backward
    float* z; int* n_out; float* loss;                              // forward
    float* dx; float* dW1; float* db1; float* dw2; float* db2;      // backward
    float* ws;
    long T, chunks;
    int D, act, splits, kper;
    int vec;                                                        // 16-byte access to x, W1 and ws
    int want_da, want_sums;
};

__device__ __forceinline__ float4 rh_ld4(const float* p, bool vec) {
    if (vec) return *reinterpret_cast<const float4*>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ void rh_st4(float* p, bool vec, const float4 v) {
    if (vec) { *reinterpret_cast<float4*>(p) = v; return; }
    p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
}
// sum over the 32 lanes that share kh (one fixed butterfly)
__device__ __forceinline__ float rh_sum32(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float rh_act(float a, int act) { return act ? fmaxf(a, 0.f) : gelu_erf(a); }
__device__ __forceinline__ float rh_act_grad(float a, int act) { return act ? (a > 0.f ? 1.f : 0.f) : gelu_erf_grad(a); }
// sigmoid(z) without overflow
__device__ __forceinline__ float rh_sigmoid(float z) {
    const float e = expf(-fabsf(z));
    return (z >= 0.f ? 1.f : e) / (1.f + e);
}

// acc0 (and acc1) += W rows x x^T over the lane's half of the contraction, k ascending.  The lane's next eight floats of x are
// in flight while the current eight feed the matrix cores: a wave has the SIMD to itself in the backward, so nothing else
// would hide the load.  half is a multiple of 8.
template <bool TWO>
__device__ __forceinline__ void rh_product(f32x16& acc0, f32x16& acc1, const float* xrow, const float* w0, const float* w1, int half,
                                           bool vec) {
    float4 xa = rh_ld4(xrow, vec), xb = rh_ld4(xrow + 4, vec);
    for (int s = 0; s < half; s += 8) {
        const float4 x0 = xa, x1 = xb;
        const int sn = s + 8 < half ? s + 8 : s;            // the last step reads its own floats again, unused
        xa = rh_ld4(xrow + sn, vec);
        xb = rh_ld4(xrow + sn + 4, vec);
        const float4 u0 = *reinterpret_cast<const float4*>(w0 + s), v0 = *reinterpret_cast<const float4*>(w0 + s + 4);
        float4 u1 = u0, v1 = v0;
        if (TWO) { u1 = *reinterpret_cast<const float4*>(w1 + s); v1 = *reinterpret_cast<const float4*>(w1 + s + 4); }
#define RH_STEP(W0, W1, X)                                                              \
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(W0, X, acc0, 0, 0, 0);              \
        if (TWO) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(W1, X, acc1, 0, 0, 0)
        RH_STEP(u0.x, u1.x, x0.x); RH_STEP(u0.y, u1.y, x0.y); RH_STEP(u0.z, u1.z, x0.z); RH_STEP(u0.w, u1.w, x0.w);
        RH_STEP(v0.x, v1.x, x1.x); RH_STEP(v0.y, v1.y, x1.y); RH_STEP(v0.z, v1.z, x1.z); RH_STEP(v0.w, v1.w, x1.w);
#undef RH_STEP
    }
}

// LDS (floats): W [RH_PT][D + 4] | b1 [RH_PT] | w2 [RH_PT] | sums [4 waves][2][RH_PT] | dz sums [4]
// two waves per SIMD (the second launch bound): two workgroups share a CU while their LDS fits (D <= 288), so one's staging,
// activations and butterflies run under the other's matrix instructions
template <bool BWD>
__global__ __launch_bounds__(256, 2) void rh_tile_kernel(RHArgs a) {
    extern __shared__ float rh_lds[];
    const int D = a.D, pitch = D + 4, half = D >> 1;
    float* Ws = rh_lds;
    float* sb1 = Ws + RH_PT * pitch;
    float* sw2 = sb1 + RH_PT;
    float* wsum = sw2 + RH_PT;
    float* wdz = wsum + 4 * 2 * RH_PT;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, kh = lane >> 5;
    const bool vec = a.vec != 0;
    const long t0 = (long)blockIdx.x * RH_TOK + wave * 32;
    const long t = t0 + c;
    const bool live = t < a.T;
    const long tc = live ? t : a.T - 1;                     // loads of rows past the end read the last row; nothing is stored
    const float* xrow = a.x + tc * D + kh * half;
    const bool on = live && (!a.active || a.active[tc] != 0);

    float dz = 0.f;
    if (BWD) {
        const int n = a.n_in[0];
        const float gs = n > 0 ? a.g[0] / (float)n : 0.f;
        const float z = a.z_in[tc];
        const float d = a.label[tc] != 0 ? 0.f - rh_sigmoid(0.f - z) : rh_sigmoid(z);      // sigmoid(z) - y
        dz = on ? gs * d : 0.f;
        if (a.want_sums) {
            const float s = rh_sum32(dz);
            if (lane == 0) wdz[wave] = s;
        }
    }
    float zacc = 0.f;
    float* part = BWD ? a.ws + a.T * D + (long)blockIdx.x * (2l * D + 4) : nullptr;

    for (int p0 = 0; p0 < D; p0 += RH_PT) {
        __syncthreads();
        // stage rows p0 .. p0 + 63 of W1 (zeros past D), b1 and w2
        const int q4 = D >> 2;
        for (int u = tid; u < RH_PT * q4; u += 256) {
            const int row = u / q4, col = (u - row * q4) << 2;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p0 + row < D) v = rh_ld4(a.W1 + (long)(p0 + row) * D + col, vec);
            *reinterpret_cast<float4*>(Ws + row * pitch + col) = v;
        }
        if (tid < RH_PT) {
            const bool ok = p0 + tid < D;
            sb1[tid] = ok ? a.b1[p0 + tid] : 0.f;
            sw2[tid] = ok ? a.w2[p0 + tid] : 0.f;
        }
        __syncthreads();
        const bool two = p0 + 32 < D;                       // the second accumulator holds rows of W1 (wave uniform)

        // a^T = b1 + W1 x^T
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc0[r] = sb1[xm_row(r, kh)];
            acc1[r] = sb1[32 + xm_row(r, kh)];
        }
        const float* w0 = Ws + c * pitch + kh * half;
        if (two) rh_product<true>(acc0, acc1, xrow, w0, w0 + 32 * pitch, half, vec);
        else rh_product<false>(acc0, acc1, xrow, w0, w0, half, vec);

        if (!BWD) {
            // rows of W1 past D are zero with b1 = w2 = 0 there: a = 0, act(0) = 0, the chain is unchanged
#pragma unroll
            for (int r = 0; r < 16; ++r) zacc = fmaf(sw2[xm_row(r, kh)], rh_act(acc0[r], a.act), zacc);
            if (two) {
#pragma unroll
                for (int r = 0; r < 16; ++r) zacc = fmaf(sw2[32 + xm_row(r, kh)], rh_act(acc1[r], a.act), zacc);
            }
            continue;
        }

        // backward: da in the accumulators' registers, its column sums, its copy for the d W1 kernel
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j == 1 && !two) break;
            f32x16& acc = j ? acc1 : acc0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int pl = 32 * j + xm_row(r, kh);
                const float av = acc[r];
                const float da = (dz * sw2[pl]) * rh_act_grad(av, a.act);
                acc[r] = da;
                if (a.want_sums) {
                    const float hz = dz * rh_act(av, a.act);
                    const float s_da = rh_sum32(da), s_hz = rh_sum32(hz);
                    if (c == 0) {
                        wsum[(wave * 2 + 0) * RH_PT + pl] = s_da;
                        wsum[(wave * 2 + 1) * RH_PT + pl] = s_hz;
                    }
                }
            }
            if (a.want_da && live) {
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const int p = p0 + 32 * j + 8 * gq + 4 * kh;        // registers 4 gq .. 4 gq + 3: rows p .. p + 3
                    if (p < D) rh_st4(a.ws + t * D + p, vec, make_float4(acc[4 * gq], acc[4 * gq + 1], acc[4 * gq + 2], acc[4 * gq + 3]));
                }
            }
        }

        // dx[t][d] (+)= sum over this tile's p of da[t][p] W1[p][d], 128 columns (four accumulators) at a time
        for (int d0 = 0; d0 < D; d0 += 128) {
            f32x16 o[4];
            int dcol[4];
            bool ok[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                ok[q] = d0 + 32 * q < D;                                  // wave uniform
                const int d = d0 + 32 * q + c;
                dcol[q] = d < D ? d : D - 1;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long tr = t0 + xm_row(r, kh);
                    o[q][r] = (p0 > 0 && ok[q] && tr < a.T) ? a.dx[tr * D + dcol[q]] : 0.f;
                }
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (j == 1 && !two) break;
                const f32x16& acc = j ? acc1 : acc0;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float* wr = Ws + (32 * j + xm_row(r, kh)) * pitch;
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (ok[q]) o[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[r], wr[dcol[q]], o[q], 0, 0, 0);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (!ok[q] || d0 + 32 * q + c >= D) continue;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long tr = t0 + xm_row(r, kh);
                    if (tr < a.T) a.dx[tr * D + dcol[q]] = o[q][r];
                }
            }
        }

        if (a.want_sums) {
            __syncthreads();
            if (tid < RH_PT && p0 + tid < D) {
                float s0 = wsum[(0 * 2 + 0) * RH_PT + tid], s1 = wsum[(0 * 2 + 1) * RH_PT + tid];
#pragma unroll
                for (int w = 1; w < 4; ++w) {
                    s0 += wsum[(w * 2 + 0) * RH_PT + tid];
                    s1 += wsum[(w * 2 + 1) * RH_PT + tid];
                }
                part[p0 + tid] = s0;
                part[D + p0 + tid] = s1;
            }
            if (p0 == 0 && tid == 0) part[2 * D] = ((wdz[0] + wdz[1]) + wdz[2]) + wdz[3];
        }
    }
    if (BWD) return;

    const float other = __shfl_xor(zacc, 32, 64);
    const float z = a.b2[0] + (kh ? other + zacc : zacc + other);
    if (kh != 0 || !live) return;
    a.z[t] = z;
    if (!a.label) return;
    const float y = a.label[t] != 0 ? 1.f : 0.f;
    const float row = fmaxf(z, 0.f) - z * y + log1pf(expf(-fabsf(z)));
    a.ws[t] = on ? row : 0.f;
}

__global__ __launch_bounds__(1024) void rh_loss_kernel(RHArgs a) {
    __shared__ float red[1024];
    __shared__ int cnt[1024];
    float acc = 0.f;
    int n = 0;
#pragma unroll 8
    for (long i = threadIdx.x; i < a.T; i += 1024) {
        acc += a.ws[i];
        n += a.active ? (a.active[i] != 0 ? 1 : 0) : 1;
    }
    red[threadIdx.x] = acc;
    cnt[threadIdx.x] = n;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { red[threadIdx.x] += red[threadIdx.x + s]; cnt[threadIdx.x] += cnt[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        a.n_out[0] = cnt[0];
        a.loss[0] = cnt[0] > 0 ? red[0] / (float)cnt[0] : 0.f;
    }
}

// one wave per (64 x 64 tile of d W1, split of the tokens): part[split][p][d] = sum over the split's tokens of da[t][p] x[t][d]
__global__ __launch_bounds__(64) void rh_dw_kernel(RHArgs a) {
    const int D = a.D, lane = threadIdx.x, c = lane & 31, kh = lane >> 5;
    const int tiles = (D + 63) >> 6;
    const int pI = (blockIdx.x / tiles) << 6, dJ = (blockIdx.x % tiles) << 6;
    const long k0 = (long)blockIdx.y * a.kper;
    const long k1 = k0 + a.kper < a.T ? k0 + a.kper : a.T;
    const float* da = a.ws;
    const bool p1 = pI + 32 < D, d1 = dJ + 32 < D;                    // wave uniform: the second half of the tile exists
    const int pa = min(pI + c, D - 1), pb = min(pI + 32 + c, D - 1);
    const int da_ = min(dJ + c, D - 1), db = min(dJ + 32 + c, D - 1);
    f32x16 o00 = zero16(), o01 = zero16(), o10 = zero16(), o11 = zero16();
    // sixteen tokens (eight steps) per round; the next round's operands are in flight while this round's feed the matrix cores
    struct Frag { float a0[8], a1[8], b0[8], b1[8]; };
    auto load = [&](Frag& f, long tt) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const long tk = tt + 2 * i + kh;
            const bool okt = tk < k1;
            const long row = (okt ? tk : k1 - 1) * D;               // every load is in bounds; a token past the split counts 0
            const float va = da[row + pa], vb = da[row + pb];
            f.a0[i] = okt ? va : 0.f;
            f.a1[i] = okt ? vb : 0.f;
            f.b0[i] = a.x[row + da_];
            f.b1[i] = a.x[row + db];
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
                if (d1) o01 = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a0[i], cur.b1[i], o01, 0, 0, 0);
                if (p1) o10 = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a1[i], cur.b0[i], o10, 0, 0, 0);
                if (p1 && d1) o11 = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a1[i], cur.b1[i], o11, 0, 0, 0);
            }
            cur = nxt;
        }
    }
    float* out = a.ws + a.T * D + a.chunks * (2l * D + 4) + (long)blockIdx.y * D * D;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int p = pI + xm_row(r, kh), d = dJ + c;
        if (p < D && d < D) out[(long)p * D + d] = o00[r];
        if (p < D && d + 32 < D) out[(long)p * D + d + 32] = o01[r];
        if (p + 32 < D && d < D) out[(long)(p + 32) * D + d] = o10[r];
        if (p + 32 < D && d + 32 < D) out[(long)(p + 32) * D + d + 32] = o11[r];
    }
}

// thread i < nW: element i of d W1, its partials in split order; then d b1 [D], d w2 [D], d b2: the chunk partials in chunk order
__global__ __launch_bounds__(256) void rh_finish_kernel(RHArgs a, long nW) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int D = a.D;
    const long stride = 2l * D + 4;
    const float* part = a.ws + a.T * D;
    if (i < nW) {
        const float* wp = part + a.chunks * stride + i;
        float s = 0.f;
#pragma unroll 8
        for (int k = 0; k < a.splits; ++k) s += wp[(long)k * D * D];
        a.dW1[i] += s;
        return;
    }
    const long e = i - nW;
    if (e > 2l * D) return;
    float* dst = e < D ? (a.db1 ? a.db1 + e : nullptr) : (e < 2l * D ? (a.dw2 ? a.dw2 + (e - D) : nullptr) : a.db2);
    if (!dst) return;
    float s = 0.f;
#pragma unroll 8
    for (long k = 0; k < a.chunks; ++k) s += part[k * stride + e];
    *dst += s;
}

}  // namespace

#define RH_ALIGNED4(p) ((uintptr_t)(p) % 4 == 0)
#define RH_ALIGNED16(p) ((uintptr_t)(p) % 16 == 0)
#define RH_CHECK_DIMS(name)                                                                                    \
    T4R_CHECK_ARG(rh_dim_ok(D), name ": D must be a multiple of 16 with 16 <= D <= 512");                     \
    T4R_CHECK_ARG(T >= 0 && T <= INT_MAX, name ": 0 <= T < 2^31 tokens");                                     \
    T4R_CHECK_ARG(act == 0 || act == 1, name ": act must be 0 (erf-GELU) or 1 (ReLU)");                       \
    if (T == 0) return 0

static size_t rh_lds_bytes(int D) { return ((size_t)RH_PT * (D + 4) + 2 * RH_PT + 8 * RH_PT + 4) * sizeof(float); }

extern "C" int t4r_rtd_head_fwd(void* stream, const float* x, const unsigned char* active, const unsigned char* label, long T, int D,
                                const float* W1, const float* b1, const float* w2, const float* b2, int act, float* z,
                                int* n_active, float* loss, float* ws) {
    RH_CHECK_DIMS("rtd_head_fwd");
    T4R_CHECK_ARG(x && W1 && b1 && w2 && b2 && z, "rtd_head_fwd: null pointer (x, W1, b1, w2, b2 or z)");
    T4R_CHECK_ARG(!label || (n_active && loss && ws), "rtd_head_fwd: labels need n_active, loss and ws");
    T4R_CHECK_ARG(RH_ALIGNED4(x) && RH_ALIGNED4(W1) && RH_ALIGNED4(b1) && RH_ALIGNED4(w2) && RH_ALIGNED4(b2) && RH_ALIGNED4(z)
                      && RH_ALIGNED4(n_active) && RH_ALIGNED4(loss) && RH_ALIGNED4(ws),
                  "rtd_head_fwd: every fp32 / int32 pointer must be 4-byte aligned");
    RHArgs a = {};
    a.x = x; a.active = active; a.label = label; a.W1 = W1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.z = z; a.n_out = n_active;
    a.loss = loss; a.ws = ws; a.T = T; a.D = D; a.act = act; a.chunks = rh_chunks(T);
    a.vec = RH_ALIGNED16(x) && RH_ALIGNED16(W1);
    const size_t smem = rh_lds_bytes(D);
    static T4rLdsAttr attr;
    t4r_ensure_dynamic_lds((const void*)rh_tile_kernel<false>, smem, attr);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rh_tile_kernel<false>, dim3((unsigned)a.chunks), dim3(256), smem, st, a);
    T4R_LAUNCH_CHECK();
    if (!label) return 0;
    hipLaunchKernelGGL(rh_loss_kernel, dim3(1), dim3(1024), 0, st, a);
    T4R_LAUNCH_CHECK();
    return 0;
}

extern "C" int t4r_rtd_head_bwd(void* stream, const float* g, const float* x, const unsigned char* active, const unsigned char* label,
                                const float* z, const int* n_active, long T, int D, const float* W1, const float* b1,
                                const float* w2, int act, float* dx, float* d_W1, float* d_b1, float* d_w2, float* d_b2,
                                float* ws) {
    RH_CHECK_DIMS("rtd_head_bwd");
    T4R_CHECK_ARG(g && x && label && z && n_active && W1 && b1 && w2 && dx && ws,
                  "rtd_head_bwd: null pointer (g, x, label, z, n_active, W1, b1, w2, dx or ws)");
    T4R_CHECK_ARG(RH_ALIGNED4(g) && RH_ALIGNED4(x) && RH_ALIGNED4(z) && RH_ALIGNED4(n_active) && RH_ALIGNED4(W1) && RH_ALIGNED4(b1)
                      && RH_ALIGNED4(w2) && RH_ALIGNED4(dx) && RH_ALIGNED4(d_W1) && RH_ALIGNED4(d_b1) && RH_ALIGNED4(d_w2)
                      && RH_ALIGNED4(d_b2) && RH_ALIGNED4(ws),
                  "rtd_head_bwd: every fp32 / int32 pointer must be 4-byte aligned");
    RHArgs a = {};
    a.g = g; a.x = x; a.active = active; a.label = label; a.z_in = z; a.n_in = n_active; a.W1 = W1; a.b1 = b1; a.w2 = w2;
    a.dx = dx; a.dW1 = d_W1; a.db1 = d_b1; a.dw2 = d_w2; a.db2 = d_b2; a.ws = ws;
    a.T = T; a.D = D; a.act = act; a.chunks = rh_chunks(T);
    a.vec = RH_ALIGNED16(x) && RH_ALIGNED16(W1) && RH_ALIGNED16(ws);
    a.want_da = d_W1 != nullptr;
    a.want_sums = d_b1 || d_w2 || d_b2;
    a.splits = (int)rh_splits(T, D);
    const long kper = (T + a.splits - 1) / a.splits;
    a.kper = (int)(kper + (kper & 1));
    const size_t smem = rh_lds_bytes(D);
    static T4rLdsAttr attr;
    t4r_ensure_dynamic_lds((const void*)rh_tile_kernel<true>, smem, attr);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rh_tile_kernel<true>, dim3((unsigned)a.chunks), dim3(256), smem, st, a);
    T4R_LAUNCH_CHECK();
    if (!a.want_da && !a.want_sums) return 0;
    const int tiles = (D + 63) / 64;
    if (a.want_da) {
        hipLaunchKernelGGL(rh_dw_kernel, dim3((unsigned)(tiles * tiles), (unsigned)a.splits), dim3(64), 0, st, a);
        T4R_LAUNCH_CHECK();
    }
    const long nW = a.want_da ? (long)D * D : 0;
    const long n = nW + (a.want_sums ? 2l * D + 1 : 0);
    hipLaunchKernelGGL(rh_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, nW);
    T4R_LAUNCH_CHECK();
    return 0;
}
