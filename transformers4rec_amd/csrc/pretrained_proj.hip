// Pretrained-embedding features (include/t4r_hip_pretrained.h): a frozen fp16 image of item vectors gathered by id inside the
// kernel that projects it, forward (16-bit matrix cores against the hi | lo planes of the fp32 weight) and backward (fp32 matrix
// cores, fixed-order split over the tokens).  gfx950 only.
//
// Forward, one wave per 32 tokens.  The product is D[p][token] = sum_e Wplane[p][e] * X[token][e]: the weight planes are the A
// operand (read from the workspace in fragment order, 1 KiB per wave-instruction), the gathered rows the B operand, so a lane
// holds ONE token's outputs in its accumulators and the LayerNorm over P is a sum over registers plus one exchange between
// the two halves of the wave.  The rows come in as 16-byte segments, 128 columns (16 segments) of each of the 32 rows per
// step and eight loads in flight per lane, into a double-buffered LDS tile of [32][16 + 1] slots (the odd pitch: the
// ds_read_b128 of the B fragments, lane (r, h) -> slot r * 17 + 2 k + h, is conflict free, as in item_h16_tile.h).
// Every accumulator element is a chain over k = 0, 16, ... in order, hi then lo, whatever the token's place in the launch.
//
// Backward, three launches: rows (LayerNorm backward per token, dZ to the workspace, column sums per token chunk), the d W
// partial of each (chunk, 32 outputs, 128 columns) on v_mfma_f32_32x32x2_f32 with X gathered again, and the sum of the partials
// in chunk order into the caller's gradients.
#include "item_h16_tile.h"
#include <limits.h>

#define PP_MAX_E 1024
#define PP_MAX_P 256
#define PP_WS_HDR 256            // bytes in front of the planes; the first float is 1 / c (t4r_hip_pretrained.h)
#define PP_MAX_CHUNKS 128
#define PP_ROWS_WAVES 16

static inline int pp_nks(int E) { return (E + 15) / 16; }
static inline int pp_npb(int P) { return (P + 31) / 32; }
static inline int pp_chunks(long T) { const long s = (T + 63) / 64; return (int)(s < 1 ? 1 : (s > PP_MAX_CHUNKS ? PP_MAX_CHUNKS : s)); }
static inline bool pp_dims_ok(int E, int P) { return E >= 1 && E <= PP_MAX_E && P >= 1 && P <= PP_MAX_P; }

extern "C" long t4r_pretrained_proj_ws_bytes(int E, int P) {
    if (!pp_dims_ok(E, P)) return 0;
    return PP_WS_HDR + (long)pp_npb(P) * pp_nks(E) * 2048;
}

extern "C" long t4r_pretrained_proj_bwd_ws_floats(long T, int E, int P) {
    if (!pp_dims_ok(E, P) || T < 0 || T > INT_MAX) return 0;
    const long S = pp_chunks(T);
    return S * (pp_npb(P) * 32L) * ((E + 127) / 128 * 128L) + (T * P + 3) / 4 * 4 + S * 6 * P;
}

namespace {

// ------------------------------------------------------------------------------------------------ the cut of W
__device__ __forceinline__ uint32_t pp_half_bits(float f) { return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)f); }

// Every workgroup takes the maximum over all of W itself (W is at most 1 MiB and stays in L2), then cuts its share of the
// fragments: for (pb, ks, lane (r, h)) the eight columns ks * 16 + 8 h + j of row pb * 32 + r, hi plane then lo plane.
__global__ __launch_bounds__(256) void pp_cut_kernel(const float* __restrict__ W, int E, int P, int nks, int npb, char* ws) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const long n = (long)P * E;
    float m = 0.f;
    if ((uintptr_t)W % 16 == 0 && n % 4 == 0) {
        const float4* W4 = reinterpret_cast<const float4*>(W);
        for (long i = tid; i < n / 4; i += 256) {
            const float4 w = W4[i];
            m = fmaxf(fmaxf(m, fmaxf(fabsf(w.x), fabsf(w.y))), fmaxf(fabsf(w.z), fabsf(w.w)));
        }
    } else {
        for (long i = tid; i < n; i += 256) m = fmaxf(m, fabsf(W[i]));
    }
    m = wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    int k = 0;
    if (m > 0.f && m <= 3.4028234e38f) {
        int ex;
        (void)frexpf(m, &ex);               // m in [2^(ex-1), 2^ex)
        k = min(15 - ex, 126);
    }
    const float c = ldexpf(1.f, k);
    if (blockIdx.x == 0 && tid == 0) *reinterpret_cast<float*>(ws) = ldexpf(1.f, -k);
    uint4* frag = reinterpret_cast<uint4*>(ws + PP_WS_HDR);
    const int total = npb * nks * 64;
    for (int idx = blockIdx.x * 256 + tid; idx < total; idx += gridDim.x * 256) {
        const int lane = idx & 63, blk = idx >> 6;          // blk = pb * nks + ks
        const int pb = blk / nks, ks = blk - pb * nks;
        const int p = pb * 32 + (lane & 31), e0 = ks * 16 + 8 * (lane >> 5);
        uint32_t hi[8], lo[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float w = (p < P && e0 + j < E) ? W[(long)p * E + e0 + j] * c : 0.f;
            const _Float16 hh = (_Float16)w;
            hi[j] = (uint32_t)__builtin_bit_cast(unsigned short, hh);
            lo[j] = pp_half_bits(w - (float)hh);
        }
        frag[(long)blk * 128 + lane] = make_uint4(hi[0] | hi[1] << 16, hi[2] | hi[3] << 16, hi[4] | hi[5] << 16, hi[6] | hi[7] << 16);
        frag[(long)blk * 128 + 64 + lane] = make_uint4(lo[0] | lo[1] << 16, lo[2] | lo[3] << 16, lo[4] | lo[5] << 16, lo[6] | lo[7] << 16);
    }
}

// ------------------------------------------------------------------------------------------------ forward
struct PPFwd {
    const uint16_t* img; long ldp; long rows; const long* ids; long T; int ids_div;
    const float* b; const float* gamma; const float* beta; float eps;
    int E, P, nks, npb;
    float* out; long ld_out; int col; float* xhat; float* rstd; const char* ws; int* err;
};

// four consecutive outputs p0 .. p0 + 3 of one row (those below P), as one 16-byte store where the address allows it
__device__ __forceinline__ void pp_store4(float* row, int p0, int P, float a, float b, float c, float d) {
    if (p0 + 3 < P && (uintptr_t)(row + p0) % 16 == 0) {
        *reinterpret_cast<float4*>(row + p0) = make_float4(a, b, c, d);
    } else {
        if (p0 < P) row[p0] = a;
        if (p0 + 1 < P) row[p0 + 1] = b;
        if (p0 + 2 < P) row[p0 + 2] = c;
        if (p0 + 3 < P) row[p0 + 3] = d;
    }
}

template <int NPB>
__global__ __launch_bounds__(64) void pp_fwd_kernel(PPFwd p) {
    __shared__ uint4 lds[2][32 * 17];
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const long tok = (long)blockIdx.x * 32 + r;
    const bool valid = tok < p.T;
    long id = p.ids[min(tok, p.T - 1) / p.ids_div];
    if (id < 0 || id >= p.rows) { if (p.err) *p.err = 1; id = 0; }      // never an address: the pad row stands in
    const int idr = (int)id;
    const uint4* frag = reinterpret_cast<const uint4*>(p.ws + PP_WS_HDR);
    const float s = *reinterpret_cast<const float*>(p.ws);
    const int nks = p.nks, nseg = 2 * nks, npb = p.npb;
    const int nchunk = (nks + 7) >> 3;

    uint4 v[8];
    auto issue = [&](int c) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = u * 64 + lane, row = idx >> 4, seg = c * 16 + (idx & 15);
            const int rid = __shfl(idr, row, 64);
            v[u] = make_uint4(0u, 0u, 0u, 0u);
            if (seg < nseg) v[u] = *reinterpret_cast<const uint4*>(p.img + (long)rid * p.ldp + seg * 8);
        }
    };
    f32x16 acc[NPB];
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[pb][e] = 0.f;

    // The weight fragments of PF k-steps are in flight at a time (registers: PF * NPB * 2 fragments = 128 VGPRs at most).  Every
    // chunk runs its eight k-steps without a branch: beyond the last k-step the LDS tile is zero, and a fragment index beyond the
    // planes is clamped to a legal one (finite times zero: the accumulators keep their bits); an output block beyond ceil(P / 32)
    // repeats the last one and is never stored.
    constexpr int PF = NPB <= 2 ? 8 : (NPB == 4 ? 4 : 2);
    uint4 fa[PF][NPB][2];
    auto load_fr = [&](int slot, int kidx) {
        const int kk = min(kidx, nks - 1);
#pragma unroll
        for (int pb = 0; pb < NPB; ++pb) {
            const uint4* fp = frag + ((long)min(pb, npb - 1) * nks + kk) * 128 + lane;
            fa[slot][pb][0] = fp[0];
            fa[slot][pb][1] = fp[64];
        }
    };
    issue(0);
    for (int c = 0; c < nchunk; ++c) {
        uint4* buf = lds[c & 1];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = u * 64 + lane;
            buf[(idx >> 4) * 17 + (idx & 15)] = v[u];
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PF; ++u) load_fr(u, c * 8 + u);
        if (c + 1 < nchunk) issue(c + 1);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const uint4 b = buf[r * 17 + 2 * ks + h];
#pragma unroll
            for (int pb = 0; pb < NPB; ++pb) {
                acc[pb] = mfma16<3>(fa[ks % PF][pb][0], b, acc[pb]);
                acc[pb] = mfma16<3>(fa[ks % PF][pb][1], b, acc[pb]);
            }
            if (ks + PF < 8) load_fr(ks % PF, c * 8 + ks + PF);
        }
    }

    // element e of acc[pb] is output pb * 32 + itk16_acc_row(e, h) of token r
    const int P = p.P;
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int pr = pb * 32 + itk16_acc_row(e, h);
            const float bias = (p.b && pr < P) ? p.b[pr] : 0.f;
            acc[pb][e] = acc[pb][e] * s + bias;
        }
    const bool ln = p.gamma != nullptr;
    float mean = 0.f, rstd = 1.f;
    if (ln) {
        float sum = 0.f;
#pragma unroll
        for (int pb = 0; pb < NPB; ++pb)
#pragma unroll
            for (int e = 0; e < 16; ++e) sum += (pb * 32 + itk16_acc_row(e, h) < P) ? acc[pb][e] : 0.f;
        sum += __shfl_xor(sum, 32, 64);
        mean = sum / (float)P;
        float var = 0.f;
#pragma unroll
        for (int pb = 0; pb < NPB; ++pb)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float d = acc[pb][e] - mean;
                var += (pb * 32 + itk16_acc_row(e, h) < P) ? d * d : 0.f;
            }
        var += __shfl_xor(var, 32, 64);
        rstd = 1.0f / sqrtf(var / (float)P + p.eps);
    }
    if (!valid) return;
    if (ln && p.rstd && h == 0) p.rstd[tok] = rstd;
    float* orow = p.out + tok * p.ld_out + p.col;
    float* xrow = (ln && p.xhat) ? p.xhat + tok * P : nullptr;
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int p0 = pb * 32 + 8 * q + 4 * h;
            if (p0 >= P) continue;
            float y[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) y[i] = acc[pb][4 * q + i];
            if (ln) {
                float xh[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    xh[i] = (y[i] - mean) * rstd;
                    const int pr = min(p0 + i, P - 1);
                    y[i] = xh[i] * p.gamma[pr] + p.beta[pr];
                }
                if (xrow) pp_store4(xrow, p0, P, xh[0], xh[1], xh[2], xh[3]);
            }
            pp_store4(orow, p0, P, y[0], y[1], y[2], y[3]);
        }
}

// ------------------------------------------------------------------------------------------------ backward
struct PPBwd {
    const uint16_t* img; long ldp; long rows; const long* ids; int T; int ids_div;
    const float* dY; long ld; int col; const float* gamma; const float* xhat; const float* rstd;
    int E, P, S, TC, PP, EP;
    float* part;        // [S][PP][EP]
    float* dZ;          // [T][P]
    double* colpart;    // [S][3][P] doubles: d gamma, d beta, d b
    float* dW; float* db; float* dgamma; float* dbeta;
};

// rows: one workgroup of 16 waves per token chunk; wave w takes tokens t_lo + w, + 16, ...; lane l the outputs l + 64 j
__global__ __launch_bounds__(64 * PP_ROWS_WAVES) void pp_bwd_rows_kernel(PPBwd p) {
    __shared__ double red[PP_ROWS_WAVES][PP_MAX_P];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int s = blockIdx.x, P = p.P;
    const int t_lo = s * p.TC, t_hi = min(p.T, t_lo + p.TC);
    const bool ln = p.gamma != nullptr;
    // the column sums run in double: a sum over tokens is then as good as its last rounding, whatever the order
    double sg[4] = {0., 0., 0., 0.}, sb[4] = {0., 0., 0., 0.}, sz[4] = {0., 0., 0., 0.};
    float gam[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) gam[j] = (ln && lane + 64 * j < P) ? p.gamma[lane + 64 * j] : 0.f;
    const float invP = 1.0f / (float)P;
    for (int t = t_lo + w; t < t_hi; t += PP_ROWS_WAVES) {
        float dy[4], xh[4], g[4], dz[4];
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int pj = lane + 64 * j;
            const bool in = pj < P;
            dy[j] = in ? p.dY[(long)t * p.ld + p.col + pj] : 0.f;
            xh[j] = (ln && in) ? p.xhat[(long)t * P + pj] : 0.f;
            g[j] = dy[j] * gam[j];
            a += g[j];
            b += g[j] * xh[j];
        }
        if (ln) {
            const float m1 = wave_sum(a) * invP, m2 = wave_sum(b) * invP, rs = p.rstd[t];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                dz[j] = rs * (g[j] - m1 - xh[j] * m2);
                sg[j] += (double)dy[j] * (double)xh[j];
                sb[j] += (double)dy[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) dz[j] = dy[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int pj = lane + 64 * j;
            if (pj < P) { sz[j] += (double)dz[j]; p.dZ[(long)t * P + pj] = dz[j]; }
        }
    }
    for (int k = 0; k < 3; ++k) {           // the 16 waves' sums of one quantity at a time: [16][256] doubles are 32 KiB
#pragma unroll
        for (int j = 0; j < 4; ++j) red[w][lane + 64 * j] = k == 0 ? sg[j] : (k == 1 ? sb[j] : sz[j]);
        __syncthreads();
        if (tid < P) {
            double acc = 0.;
#pragma unroll
            for (int ww = 0; ww < PP_ROWS_WAVES; ++ww) acc += red[ww][tid];
            p.colpart[((long)s * 3 + k) * P + tid] = acc;
        }
        __syncthreads();
    }
}

// d W partial of (128 columns, 32 outputs, chunk): D[p][e] += dZ[t][p] * X[t][e], two tokens per instruction.  Lane (c, kh) holds
// columns e0 .. e0 + 3 = 128 g + 4 c .. + 3 of token t + kh in one 8-byte load; tile j takes column 4 c + j, so that the four
// accumulators of a lane are four consecutive columns of d W: a 16-byte store.
__global__ __launch_bounds__(64) void pp_bwd_dw_kernel(PPBwd p) {
    const int lane = threadIdx.x, c = lane & 31, kh = lane >> 5;
    const int pb = blockIdx.y, s = blockIdx.z, P = p.P;
    const int e0 = blockIdx.x * 128 + 4 * c;
    const bool e_in = e0 < (p.E + 15) / 16 * 16;           // inside the image's k extent (<= ldp, a multiple of 8)
    const int pc = min(pb * 32 + c, P - 1);
    const int t_lo = s * p.TC, t_hi = min(p.T, t_lo + p.TC);
    f32x16 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    const bool div1 = p.ids_div == 1;
#pragma unroll 8
    for (int tb = t_lo; tb < t_hi; tb += 2) {
        const int t = tb + kh;
        const bool ok = t < t_hi;
        const int tt = ok ? t : t_lo;
        long id = p.ids[div1 ? tt : tt / p.ids_div];
        if (id < 0 || id >= p.rows) id = 0;
        const float a = ok ? p.dZ[(long)tt * P + pc] : 0.f;
        uint2 x = make_uint2(0u, 0u);
        if (ok && e_in) x = *reinterpret_cast<const uint2*>(p.img + id * p.ldp + e0);
        const float b0 = (float)__builtin_bit_cast(_Float16, (unsigned short)(x.x & 0xffffu));
        const float b1 = (float)__builtin_bit_cast(_Float16, (unsigned short)(x.x >> 16));
        const float b2 = (float)__builtin_bit_cast(_Float16, (unsigned short)(x.y & 0xffffu));
        const float b3 = (float)__builtin_bit_cast(_Float16, (unsigned short)(x.y >> 16));
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[1], 0, 0, 0);
        acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b2, acc[2], 0, 0, 0);
        acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b3, acc[3], 0, 0, 0);
    }
    float* base = p.part + ((long)s * p.PP + pb * 32) * p.EP + e0;
#pragma unroll
    for (int e = 0; e < 16; ++e)
        *reinterpret_cast<float4*>(base + (long)itk16_acc_row(e, kh) * p.EP) = make_float4(acc[0][e], acc[1][e], acc[2][e], acc[3][e]);
}

// the partials in chunk order, then one add into the caller's gradient
__global__ __launch_bounds__(256) void pp_bwd_reduce_kernel(PPBwd p) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long nW = (long)p.P * p.E;
    if (i < nW) {
        if (!p.dW) return;
        const int pr = (int)(i / p.E), e = (int)(i - (long)pr * p.E);
        float acc = 0.f;
        for (int s = 0; s < p.S; ++s) acc += p.part[((long)s * p.PP + pr) * p.EP + e];
        p.dW[i] += acc;
    } else if (i < nW + 3 * p.P) {
        const int k = (int)((i - nW) / p.P), pj = (int)(i - nW - (long)k * p.P);
        float* dst = k == 0 ? p.dgamma : (k == 1 ? p.dbeta : p.db);
        if (!dst || (k < 2 && !p.gamma)) return;
        double acc = 0.;
        for (int s = 0; s < p.S; ++s) acc += p.colpart[((long)s * 3 + k) * p.P + pj];
        dst[pj] += (float)acc;
    }
}

}  // namespace

// the arguments both directions share
#define PP_CHECK_COMMON(name)                                                                                                       \
    T4R_CHECK_ARG(E >= 1 && E <= PP_MAX_E, name ": 1 <= E <= 1024");                                                                \
    T4R_CHECK_ARG(P >= 1 && P <= PP_MAX_P, name ": 1 <= P <= 256");                                                                 \
    T4R_CHECK_ARG(dtype != 2, name ": a bf16 image is not supported: pack the table as fp16 (dtype 3)");                            \
    T4R_CHECK_ARG(dtype == 3, name ": dtype is 3 (fp16), the code of T4R_GEMM_PREC");                                               \
    T4R_CHECK_ARG(image && ldp >= itk16_image_ld(E) && ldp % 8 == 0 && (uintptr_t)image % 16 == 0,                                  \
                  name ": image rows must be 16-byte aligned with pitch >= t4r_item_table_image_ld(E)");                            \
    T4R_CHECK_ARG(rows >= 1 && rows <= INT_MAX, name ": 1 <= rows < 2^31");                                                         \
    T4R_CHECK_ARG(T >= 0 && T <= INT_MAX, name ": 0 <= T < 2^31");                                                                  \
    T4R_CHECK_ARG(ids_div >= 1 && T % ids_div == 0, name ": ids_div must be >= 1 and divide T");                                    \
    T4R_CHECK_ARG(ids || T == 0, name ": ids is null")

extern "C" int t4r_pretrained_proj_fwd(void* stream, int dtype, const void* image, long ldp, long rows, const long* ids, long T,
                                       int ids_div, const float* W, const float* b, const float* gamma, const float* beta, float eps,
                                       int E, int P, float* out, long ld_out, int col, float* xhat, float* rstd, void* ws,
                                       int* err_flag) {
    PP_CHECK_COMMON("pretrained_proj_fwd");
    T4R_CHECK_ARG(W && out, "pretrained_proj_fwd: W or out is null");
    T4R_CHECK_ARG((gamma == nullptr) == (beta == nullptr), "pretrained_proj_fwd: gamma and beta come together");
    T4R_CHECK_ARG(col >= 0 && ld_out >= (long)col + P, "pretrained_proj_fwd: ld_out below col + P");
    T4R_CHECK_ARG(ws && (uintptr_t)ws % 16 == 0, "pretrained_proj_fwd: workspace null or not 16-byte aligned");
    if (T == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int nks = pp_nks(E), npb = pp_npb(P);
    const int cut_wgs = (int)min(32L, max(1L, (long)P * E / 8192));
    hipLaunchKernelGGL(pp_cut_kernel, dim3(cut_wgs), dim3(256), 0, st, W, E, P, nks, npb, (char*)ws);
    T4R_LAUNCH_CHECK();
    PPFwd p = {};
    p.img = (const uint16_t*)image; p.ldp = ldp; p.rows = rows; p.ids = ids; p.T = T; p.ids_div = ids_div;
    p.b = b; p.gamma = gamma; p.beta = beta; p.eps = eps; p.E = E; p.P = P; p.nks = nks; p.npb = npb;
    p.out = out; p.ld_out = ld_out; p.col = col; p.xhat = xhat; p.rstd = rstd; p.ws = (const char*)ws; p.err = err_flag;
    const dim3 grid((unsigned)((T + 31) / 32));
    if (npb <= 1) hipLaunchKernelGGL(pp_fwd_kernel<1>, grid, dim3(64), 0, st, p);
    else if (npb <= 2) hipLaunchKernelGGL(pp_fwd_kernel<2>, grid, dim3(64), 0, st, p);
    else if (npb <= 4) hipLaunchKernelGGL(pp_fwd_kernel<4>, grid, dim3(64), 0, st, p);
    else hipLaunchKernelGGL(pp_fwd_kernel<8>, grid, dim3(64), 0, st, p);
    T4R_LAUNCH_CHECK();
    return 0;
}

extern "C" int t4r_pretrained_proj_bwd(void* stream, int dtype, const void* image, long ldp, long rows, const long* ids, long T,
                                       int ids_div, const float* dY, long ld, int col, const float* gamma, const float* xhat,
                                       const float* rstd, int E, int P, float* dW, float* db, float* dgamma, float* dbeta,
                                       float* ws) {
    PP_CHECK_COMMON("pretrained_proj_bwd");
    T4R_CHECK_ARG(dY && col >= 0 && ld >= (long)col + P, "pretrained_proj_bwd: dY null or ld below col + P");
    T4R_CHECK_ARG(!gamma || (xhat && rstd), "pretrained_proj_bwd: with gamma, the forward's xhat and rstd are required");
    T4R_CHECK_ARG(ws && (uintptr_t)ws % 16 == 0, "pretrained_proj_bwd: workspace null or not 16-byte aligned");
    if (T == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    PPBwd p = {};
    p.img = (const uint16_t*)image; p.ldp = ldp; p.rows = rows; p.ids = ids; p.T = (int)T; p.ids_div = ids_div;
    p.dY = dY; p.ld = ld; p.col = col; p.gamma = gamma; p.xhat = xhat; p.rstd = rstd; p.E = E; p.P = P;
    p.S = pp_chunks(T); p.TC = (int)((T + p.S - 1) / p.S); p.PP = pp_npb(P) * 32; p.EP = (E + 127) / 128 * 128;
    p.part = ws;
    p.dZ = p.part + (long)p.S * p.PP * p.EP;
    p.colpart = reinterpret_cast<double*>(p.dZ + (T * P + 3) / 4 * 4);
    p.dW = dW; p.db = db; p.dgamma = dgamma; p.dbeta = dbeta;
    hipLaunchKernelGGL(pp_bwd_rows_kernel, dim3(p.S), dim3(64 * PP_ROWS_WAVES), 0, st, p);
    T4R_LAUNCH_CHECK();
    if (dW) {
        hipLaunchKernelGGL(pp_bwd_dw_kernel, dim3(p.EP / 128, pp_npb(P), p.S), dim3(64), 0, st, p);
        T4R_LAUNCH_CHECK();
    }
    const long n = (long)P * E + 3 * P;
    hipLaunchKernelGGL(pp_bwd_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p);
    T4R_LAUNCH_CHECK();
    return 0;
}
