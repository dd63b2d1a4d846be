"""Plain-torch restatement of the two-way fp16 split ARITHMETIC of the XLNet body (csrc/xlnet_fused.h: pow2_scale, cut2h,
product3h; csrc/xlnet_fused.hip: the scale policies of the feed-forward pair), and the error budget that follows from it.
Not a restatement of the kernels: no tiles, no LDS, no lanes -- only which number is rounded where, and with which scale.

The arithmetic
--------------
An fp32 operand x is positioned by a power of two s and cut into two fp16 pieces, both cuts round to nearest even:
    v = x s,   hi = fp16(v),   lo = fp16(v - hi)            (v - hi is exact in fp32)
The scale comes from one of three policies:
    token rows        s = pow2_scale(max |row|)             the row's own maximum lands in [2^13, 2^14)
    weights           s = pow2_scale(max |matrix|)          one per source matrix
    chained rows      s = pow2_scale(bound[t])              an a-priori per-token bound, known before the product before it ran:
                          FF activations   (D max|W1| max|h1[t]| + max|b1|) / keep,   max|W1| rounded up to 2^14 / s_W1
                          d pre rows       1.13 / keep  D max|W2| max|d ffout[t]|,      max|W2| rounded up to 2^14 / s_W2
with pow2_scale(m) = 2^min(14 - e, 100) for m = f 2^e, f in [0.5, 1), and 1 for m = 0, inf, NaN.
A product y[t, f] = sum_k a[t, k] w[k, f] keeps three of the four piece products, fp32 accumulation in the matrix cores,
smallest first, then leaves the scaled domain by the exact factor 1 / (s_a[t] s_w):
    acc = sum_k (lo_a hi_w + hi_a lo_w + hi_a hi_w),    y = acc / (s_a s_w)

Error of one operand (scaled units, |v| < 2^14 so nothing overflows fp16's 65504)
    hi is normal (|v| >= 2^-14, exponent e):  |lo| <= 2^(e-11) <= 2^-11 |v|, and fp16(lo) is off by at most
        max(2^(e-22), 2^-25): half an ulp of lo, or half the subnormal spacing 2^-24 once lo itself is below 2^-14.
    hi is subnormal: |v - hi| <= 2^-25, |lo| <= 2^-25 and fp16(lo) is again off by at most 2^-25.
    => |hi + lo - v| <= max(2^-22 |v|, 2^-25) =: d(v),      |lo| <= max(2^-11 |v|, 2^-25) =: l(v),     d(0) = l(0) = 0.
The RELATIVE term holds down to |v| = 2^-3: 2^16 below a maximum (or bound) that the scale put at the bottom of its window
[2^13, 2^14), 2^17 below one at its top -- the window the kernels' comment promises is "2^16 to 2^17", and the tests place
their in-window channel 2^12 and their out-of-window channel 2^22 below the row's largest.  Below it the ABSOLUTE floor
2^-25 (2^-25 / s in value units) takes over, and nothing further down is lost faster than the floor.

split_bound(a, w, sa, sw): per element of y, with A = |a|, W = |w|, da = d(a sa) / sa, la = l(a sa) / sa (dw, lw alike)
    representation   sum_k da (W + dw) + A dw            both operands' cuts, first order and their cross term
                     + sum_k la lw                        the dropped lo lo product
    accumulation     3 K 2^-23 sum_k A W                  3 K fp32 additions of exact products (11 x 11 bits fit 24); one ULP
                                                          each, not half, as the matrix cores need not round to nearest
    floor            inside da, dw, la, lw: the max(., 2^-25 / s) branch
    chained input    sum_k ea W                           when a itself carries an error ea from the stage before (A := A + ea)

The feed-forward block, forward (u = 2^-24, every line per element, |.| element-wise)
    ffpre = h1 W1^T + b1          e_pre  = split_bound(h1, W1^T, s_row, s_W1) + u (|pre| + |b1|)
    ffact = gelu(pre) m_a         e_act  = m_a (1.13 e_pre + 2^-22 |pre| + 2^-23 |gelu|) + u |act| + 2^-126
                                  (|gelu'| <= 1.13; erf_bf is good to an ULP of 1, so gelu is off by <= 2^-22 |x| / 2 + roundings;
                                   2^-126: a result below fp32's normal range may be flushed)
    ffout = act W2^T + b2         e_out  = split_bound(act, W2^T, s_bound, s_W2, ea = e_act) + u (|ffout| + |b2|)
    hout  = LN(ffout m_o + h1)    e_hout = ln_fwd_bound(x, e_x = m_o e_out + u |x|): the LayerNorm Jacobian
                                  |d y_i / d x_j| <= rs |g_i| (delta_ij + 1/D + |xh_i xh_j| / D) applied to e_x, plus the fp32
                                  evaluation of the LayerNorm itself (ln_fwd_bound).
Backward (xh, rs as saved by the forward, so they carry e_x)
    d x    = rs (gg - mean gg - xh mean(gg xh)), gg = dy g:        ln_bwd_bound (propagated e_x + fp32 evaluation)
    d ffout = d x m_o                                              e_dfo = m_o e_dx
    d act  = d ffout W2          e_dact = split_bound(d ffout, W2, s_row, s_W2, ea = e_dfo)
    d pre  = d act gelu'(pre) m_a   e_dpre = m_a (1.13 e_dact + |d act| (0.8 e_pre + 2^-21)) + u |d pre| + 2^-126
                                  (|gelu''| <= 0.8; cdf and x pdf of gelu_erf_grad are each good to ~2^-22 absolute)
    d h1   = d x + d pre W1      e_dh1 = e_dx + split_bound(d pre, W1, s_bound, s_W1, ea = e_dpre) + u |d h1|
The two backward scales depend on the DEVICE's max |d ffout[t]|, which may sit across a power of two from the reference's:
their floor is taken at half the restated scale.

What is not scale-free.  The products are bilinear, the block is not: gelu' has curvature 0.8 around 0, so an absolute error
e_pre ~ 2^-22 max |pre| moves d pre by 0.8 e_pre |d act| wherever |pre| < 3.  With b1 scaled to thousands (family A, sx sw =
3500) max |pre| is 10^4 and that is 10^-4 of the largest d pre in ANY fp32 evaluation (the fp32 chain on the CPU: 4e-5 at
D = 128, the kernels 4.6e-5).  e_dpre carries the term; the tensor-relative limits are asserted on what the project asserts
them on at unit scale (the saved forward tensors, d h1, the bias / LayerNorm sums, the two weight-gradient contractions) and
the two row operands d ffout / d pre are held per row.

Behind the softmax (the one-kernel attention block: q | k | v on the split, the core and the o-projection in exact fp32)
    s_ij = ((q_i + r_w) k_j + (q_i + r_r) k_r[j + L - i]) / sqrt(d)
    e_s,ij = sum_h (e_q,ih (|k_jh| + e_k,jh + |k_r,mh|) + (|q_ih| + |r_w,h|) e_k,jh) / sqrt(d)        the projections' errors
             + (2 d + 6) u sum_h ((|q_ih| + |r_w,h|) |k_jh| + (|q_ih| + |r_r,h|) |k_r,mh|) / sqrt(d)     the fp32 score itself
    with D_i = max_j e_s,ij over the live keys (a masked key has probability exactly 0 on both sides):
    P~_ij / P_ij = exp(d_ij) / sum_j' P_ij' exp(d_ij') lies in [exp(-2 D_i), exp(2 D_i)], so with a_i = expm1(2 D_i) + (L + 8) u
    (the exponentials, their sum and the division in fp32)
    lse      e_lse,i = D_i + (L + 8) u + u |lse_i|
    attn_vec e_av,i  = a_i sum_j P_ij |v_j| + (1 + a_i) sum_j P_ij e_v,j + (L + 2) u sum_j P_ij |v_j|
    ao = av o^T      e_ao = e_av |o|^T + (D + 2) u |av| |o|^T
    h1, mean, rstd   the LayerNorm propagation of e_x = e_ao + u |x|, x = ao + h, as in the feed-forward block.
All of them are held per row.  The tensor-relative 6e-6 that tests/test_attn_block_gpu.py asserts at unit scale presupposes
scores of order 1: fp32 rounds a score s to within u |s| at best, and the output moves by expm1 of twice that.  Where
u max_j |s_ij| exceeds the limit itself (|s| > 6e-6 / u = 100: token rows 2^5 and more above their session's others -- there
lse reaches 10^4 and the softmax is one-hot), no fp32 evaluation can promise 6e-6, the fp32 evaluation of the reference on the
CPU included (1.7e-5 on attn_vec at d_model 128).  The limit is therefore asserted over the rows whose scores stay within 100,
at its unit-scale value, and the rows beyond are held to the per-row bound alone (attn_bounds returns the mask).

What the bound buys.  All terms are relative to sum_k |a[t, k]| |w[k, f]| of the SAME row t, or absolute in the row's own
scaled units.  A scale shared between rows (per 16-row tile, per tensor) puts a row that lies 2^-20 and more below its
neighbours under the floor of THEIR scale: its error becomes 2^-25 / s_neighbour, many orders above this bound.  That is what
the per-row-magnitude family (B) observes; tests/test_body_split_cpu.py shows that both variants leave the bound there.
"""
import math

import torch

F64, F32 = torch.float64, torch.float32
U = 2.0 ** -24
FP32_MIN_NORMAL = 2.0 ** -126
FP32_MAX = 3.4028234663852886e38


# ------------------------------------------------------------------------------------------------ the arithmetic
def pow2_scale(m):
    """csrc/xlnet_fused.h pow2_scale, element-wise on an fp32 tensor"""
    m = torch.as_tensor(m, dtype=F32)
    ok = (m > 0) & (m < 3e38)
    _, e = torch.frexp(torch.where(ok, m, torch.ones_like(m)))
    s = torch.ldexp(torch.ones_like(m), torch.clamp(14 - e, max=100))
    return torch.where(ok, s, torch.ones_like(m))


def cut2(v):
    """two fp16 pieces of an already scaled fp32 tensor, returned as fp32 (cut2h)"""
    hi = v.to(torch.float16).to(F32)
    lo = (v - hi).to(torch.float16).to(F32)
    return hi, lo


def split_mm(a, w, sa, sw):
    """y = a @ w on the two-way split: a [T, K] fp32 with scales sa [T], w [K, F] fp32 with the scale sw"""
    sa = torch.as_tensor(sa, dtype=F32).expand(a.shape[0]).reshape(-1, 1)
    sw = torch.as_tensor(sw, dtype=F32)
    ah, al = cut2(a * sa)
    wh, wl = cut2(w * sw)
    acc = al @ wh
    acc = acc + ah @ wl
    acc = acc + ah @ wh
    return acc * ((1.0 / sa) * (1.0 / sw))


# ------------------------------------------------------------------------------------------------ the scale policies
def row_amax(a, mode="row"):
    """max |row| as the policy sees it: the row's own ('row', the project's), its 16-row tile's, or the tensor's"""
    m = a.abs().amax(dim=1)
    if mode == "row":
        return m
    if mode == "tensor":
        return m.amax().expand_as(m).clone()
    assert mode == "tile"
    T = m.shape[0]
    pad = torch.cat([m, m.new_zeros((-T) % 16)]).view(-1, 16)
    return pad.amax(dim=1, keepdim=True).expand(-1, 16).reshape(-1)[:T].clone()


def matrix_scale(w):
    return pow2_scale(w.abs().amax())


def act_scale(h1max, w1, b1, inv_keep, D):
    """the a-priori scale of a token's FF activation row (ff_fwd_body)"""
    w1max = torch.tensor(16384.0, dtype=F32) / matrix_scale(w1)
    return pow2_scale((torch.tensor(float(D), dtype=F32) * w1max * h1max + b1.abs().amax()) * torch.tensor(inv_keep, dtype=F32))


def dpre_scale(dfomax, w2, inv_keep, D):
    """the a-priori scale of a token's d pre row (xlnet_ff_bwd_kernel)"""
    w2max = torch.tensor(16384.0, dtype=F32) / matrix_scale(w2)
    return pow2_scale(torch.tensor(1.13, dtype=F32) * torch.tensor(inv_keep, dtype=F32) * torch.tensor(float(D), dtype=F32)
                      * w2max * dfomax)


# ------------------------------------------------------------------------------------------------ the bound
def _piece_err(x, s, extra=None):
    """d(.) and l(.) of the docstring in value units; x fp64 magnitudes, s broadcastable scales"""
    s = torch.as_tensor(s, dtype=F64)
    floor = (2.0 ** -25) / s
    live = x > 0 if extra is None else (x > 0) | (extra > 0)
    z = torch.zeros_like(x)
    return torch.where(live, torch.maximum(x * 2.0 ** -22, floor), z), torch.where(live, torch.maximum(x * 2.0 ** -11, floor), z)


def split_bound(a, w, sa, sw, ea=None):
    """per-element bound [T, F] on |split_mm(a, w, sa, sw) - a @ w| (module docstring).  a, w: the exact operands; ea: the
    error a already carries"""
    A, W = a.to(F64).abs(), w.to(F64).abs()
    sa = torch.as_tensor(sa, dtype=F64).expand(A.shape[0]).reshape(-1, 1)
    if ea is not None:
        A = A + ea
    da, la = _piece_err(A, sa, ea)
    dw, lw = _piece_err(W, float(sw))
    rep = da @ (W + dw) + A @ dw + la @ lw
    acc = 3 * a.shape[1] * 2.0 ** -23 * (A @ W)
    chain = ea @ W if ea is not None else 0.0
    return rep + acc + chain


def ln_stats(x, eps):
    mu = x.mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    return mu, rs, (x - mu) * rs


def ln_fwd_bound(x, ex, gamma, beta, eps):
    """error of y = LN(x) g + b evaluated in fp32 on an input that is off by ex"""
    D = x.shape[-1]
    mu, rs, xh = ln_stats(x, eps)
    g, y = gamma.abs(), xh * gamma + beta
    prop = rs * g * (ex + ex.mean(-1, keepdim=True) + xh.abs() * (xh.abs() * ex).mean(-1, keepdim=True))
    xmax = x.abs().amax(-1, keepdim=True)
    rnd = U * (rs * g * (8 * xmax + 4 * (x - mu).abs()) + (D / 2 + 4) * (g * xh.abs()) + 2 * (y.abs() + beta.abs()))
    return prop + rnd


def ln_bwd_bound(x, ex, dy, gamma, eps):
    """error of d x = rs (gg - mean gg - xh mean(gg xh)) in fp32, xh and rs from an x that is off by ex"""
    D = x.shape[-1]
    mu, rs, xh = ln_stats(x, eps)
    gg = (dy * gamma).abs()
    xmax = x.abs().amax(-1, keepdim=True)
    exh = rs * (ex + ex.mean(-1, keepdim=True) + xh.abs() * (xh.abs() * ex).mean(-1, keepdim=True)) \
        + U * (8 * xmax * rs + (D / 2 + 6) * xh.abs())
    ers = rs * (xh.abs() * ex).mean(-1, keepdim=True) + U * (D / 2 + 4)          # relative error of rs
    s2 = (dy * gamma * xh).mean(-1, keepdim=True).abs()
    dx = rs * (dy * gamma - (dy * gamma).mean(-1, keepdim=True) - xh * (dy * gamma * xh).mean(-1, keepdim=True))
    size = rs * (gg + gg.mean(-1, keepdim=True) + xh.abs() * (gg * xh.abs()).mean(-1, keepdim=True))
    return ers * dx.abs() + rs * (exh * s2 + xh.abs() * (gg * exh).mean(-1, keepdim=True)) + U * (math.log2(D) + 8) * size


def attn_bounds(p, h, kr, B, L, n, ref, key_len=None, eps=0.03, score_limit=6e-6):
    """per-element bounds behind the softmax of the attention block (module docstring) for lse [B, n, L], av, ao, h1 [T, D],
    mean, rstd [T, 1], and `benign` [T]: the token rows whose scores stay within score_limit / u in every head.
    p, h, kr [2L, D]: fp64 copies of the fp32 inputs; ref: the fp64 evaluation (tests/test_attn_block_gpu.py: reference)"""
    T, D = h.shape
    dh = D // n
    heads = lambda t: t.view(B, L, n, dh).permute(0, 2, 1, 3)                # [T, D] -> [B, n, L, dh]
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(T, D)
    hs = pow2_scale(row_amax(h.to(F32)))
    q, k, v = (heads(ref["qkv"][z]) for z in range(3))
    e_q, e_k, e_v = (heads(split_bound(h, p[nm].reshape(D, D), hs, matrix_scale(p[nm].to(F32))) + U * ref["qkv"][z].abs())
                     for z, nm in enumerate("qkv"))
    krh = kr.view(2 * L, n, dh).permute(1, 0, 2).abs()                       # [n, 2L, dh]
    rw, rr = p["r_w_bias"].abs()[None, :, None, :], p["r_r_bias"].abs()[None, :, None, :]
    i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
    idx = (j + L - i).expand(B, n, L, L)
    shift = lambda t: torch.gather(t, 3, idx)                                # [B, n, L, 2L] -> [B, n, L, L]
    mm = lambda a, b: torch.einsum("bnih,bnjh->bnij", a, b)
    mr = lambda a: shift(torch.einsum("bnih,nmh->bnim", a, krh))
    e_s = (mm(e_q, k.abs() + e_k) + mr(e_q) + mm(q.abs() + rw, e_k)
           + (2 * dh + 6) * U * (mm(q.abs() + rw, k.abs()) + mr(q.abs() + rr))) / math.sqrt(dh)
    sc = (mm(q + p["r_w_bias"][None, :, None, :], k)
          + shift(torch.einsum("bnih,nmh->bnim", q + p["r_r_bias"][None, :, None, :], kr.view(2 * L, n, dh).permute(1, 0, 2)))) / math.sqrt(dh)
    live = torch.ones(B, 1, L, L, dtype=torch.bool)
    if key_len is not None:
        live = ~((j[None] >= key_len.view(B, 1, 1)) & (j != i)[None])[:, None]
    live = live.expand(B, n, L, L)
    Dl = torch.where(live, e_s, torch.zeros_like(e_s)).amax(-1)              # [B, n, L]
    smax = torch.where(live, sc.abs(), torch.zeros_like(sc)).amax(-1)
    P = torch.softmax(torch.where(live, sc, torch.full_like(sc, -1e30)), -1)
    a = (torch.expm1(2 * Dl) + (L + 8) * U)[..., None]                       # [B, n, L, 1]
    Pv = torch.einsum("bnij,bnjh->bnih", P, v.abs())
    e_av = rows(a * Pv + (1 + a) * torch.einsum("bnij,bnjh->bnih", P, e_v) + (L + 2) * U * Pv)
    o = p["o"].reshape(D, D).abs()
    e_ao = e_av @ o.t() + (D + 2) * U * (ref["av"].abs() @ o.t())
    x = ref["ao"] + h
    e_x = e_ao + U * x.abs()
    mu, rs, xh = ln_stats(x, eps)
    return dict(lse=Dl + (L + 8) * U + U * ref["lse"].abs(), av=e_av, ao=e_ao,
                h1=ln_fwd_bound(x, e_x, p["ln_w"], p["ln_b"], eps),
                mean=e_x.mean(-1, keepdim=True) + 8 * U * x.abs().amax(-1, keepdim=True),
                rstd=rs * (rs * (xh.abs() * e_x).mean(-1, keepdim=True) + U * (D / 2 + 4)),
                benign=(smax.amax(1) * U <= score_limit).reshape(T), smax=smax)


# ------------------------------------------------------------------------------------------------ the FF chain
def gelu(x):
    return torch.nn.functional.gelu(x)


def gelu_grad(x):
    return 0.5 * torch.erfc(-x * math.sqrt(0.5)) + x * torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))


class Exact:
    """products as they are (fp64 reference, or the fp32 chain)"""

    def __init__(self, dtype):
        self.dtype = dtype

    def ff1(self, h1, p): return h1 @ p["w1"].t()
    def ff2(self, act, h1, p): return act @ p["w2"].t()
    def dact(self, dfo, p): return dfo @ p["w2"]
    def dh1(self, dpre, dfo, p): return dpre @ p["w1"]


class Split:
    """the four products on the two-way split with the project's policies (mode = 'row') or a broken token policy"""
    dtype = F32

    def __init__(self, D, inv_keep=1.0, mode="row"):
        self.D, self.inv_keep, self.mode = D, inv_keep, mode

    def ff1(self, h1, p):
        return split_mm(h1, p["w1"].t(), pow2_scale(row_amax(h1, self.mode)), matrix_scale(p["w1"]))

    def ff2(self, act, h1, p):
        return split_mm(act, p["w2"].t(), act_scale(row_amax(h1, self.mode), p["w1"], p["b1"], self.inv_keep, self.D),
                        matrix_scale(p["w2"]))

    def dact(self, dfo, p):
        return split_mm(dfo, p["w2"], pow2_scale(row_amax(dfo, self.mode)), matrix_scale(p["w2"]))

    def dh1(self, dpre, dfo, p):
        return split_mm(dpre, p["w1"], dpre_scale(row_amax(dfo, self.mode), p["w2"], self.inv_keep, self.D),
                        matrix_scale(p["w1"]))


FF_KEYS = ("w1", "b1", "w2", "b2", "ff_ln_w", "ff_ln_b")
FF_ROW_OUTPUTS = ("ffpre", "ffact", "ffout", "hout", "dffout", "dpre", "dh1")


def ff_chain(mm, h1, p, dy, ma, mo, eps=0.03):
    """the feed-forward block and its backward, every product through `mm` (Exact or Split), the rest in mm.dtype.
    ma [T, 4D], mo [T, D]: dropout masks times 1 / keep (ones without dropout)"""
    dt = mm.dtype
    h1, dy, ma, mo = h1.to(dt), dy.to(dt), ma.to(dt), mo.to(dt)
    p = {k: p[k].to(dt) for k in FF_KEYS}
    pre = mm.ff1(h1, p) + p["b1"]
    act = gelu(pre) * ma
    ffo = mm.ff2(act, h1, p) + p["b2"]
    x = ffo * mo + h1
    mu, rs, xh = ln_stats(x, eps)
    hout = xh * p["ff_ln_w"] + p["ff_ln_b"]
    gg = dy * p["ff_ln_w"]
    dx = rs * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True))
    dfo = dx * mo
    dact = mm.dact(dfo, p)
    dpre = dact * gelu_grad(pre) * ma
    dh1 = dx + mm.dh1(dpre, dfo, p)
    return dict(ffpre=pre, ffact=act, ffout=ffo, hout=hout, dffout=dfo, dpre=dpre, dh1=dh1, x=x, dact=dact, mean=mu, rstd=rs,
                d_ff_ln_w=(dy * xh).sum(0), d_ff_ln_b=dy.sum(0), d_b2=dfo.sum(0), d_b1=dpre.sum(0),
                d_w2=dfo.t() @ act, d_w1=dpre.t() @ h1)


def ff_bounds(ref, h1, p, dy, ma, mo, inv_keep=1.0, eps=0.03):
    """per-element bounds for FF_ROW_OUTPUTS from the fp64 evaluation `ref` = ff_chain(Exact(F64), ...) (module docstring)"""
    D = h1.shape[1]
    h32 = h1.to(F32)
    p32 = {k: p[k].to(F32) for k in FF_KEYS}
    w1, w2 = p["w1"].to(F64), p["w2"].to(F64)
    ma, mo = ma.to(F64), mo.to(F64)
    s_w1, s_w2 = float(matrix_scale(p32["w1"])), float(matrix_scale(p32["w2"]))
    hmax = row_amax(h32)
    pre, act, ffo, x = ref["ffpre"], ref["ffact"], ref["ffout"], ref["x"]
    e_pre = split_bound(h1, w1.t(), pow2_scale(hmax), s_w1) + U * (pre.abs() + p["b1"].abs())
    e_act = ma * (1.13 * e_pre + 2.0 ** -22 * pre.abs() + 2.0 ** -23 * gelu(pre).abs()) + U * act.abs() + FP32_MIN_NORMAL
    e_out = split_bound(act, w2.t(), act_scale(hmax, p32["w1"], p32["b1"], inv_keep, D), s_w2, ea=e_act) \
        + U * (ffo.abs() + p["b2"].abs())
    e_x = mo * e_out + U * x.abs()
    e_hout = ln_fwd_bound(x, e_x, p["ff_ln_w"].to(F64), p["ff_ln_b"].to(F64), eps)
    mu, rs, xh = ln_stats(x, eps)             # the saved statistics: the same propagation, without gamma
    e_mean = e_x.mean(-1, keepdim=True) + 8 * U * x.abs().amax(-1, keepdim=True)
    e_rstd = rs * (rs * (xh.abs() * e_x).mean(-1, keepdim=True) + U * (D / 2 + 4))
    e_dx = ln_bwd_bound(x, e_x, dy.to(F64), p["ff_ln_w"].to(F64), eps)
    e_dfo = mo * e_dx
    dfomax = row_amax(ref["dffout"].to(F32))
    e_dact = split_bound(ref["dffout"], w2, pow2_scale(dfomax) * 0.5, s_w2, ea=e_dfo)
    e_dpre = ma * (1.13 * e_dact + ref["dact"].abs() * (0.8 * e_pre + 2.0 ** -21)) + U * ref["dpre"].abs() + FP32_MIN_NORMAL
    e_dpre = torch.where((ref["dffout"].abs().amax(1, keepdim=True) > 0).expand_as(e_dpre), e_dpre, torch.zeros_like(e_dpre))
    e_dh1 = e_dx + split_bound(ref["dpre"], w1, dpre_scale(dfomax, p32["w2"], inv_keep, D) * 0.5, s_w1, ea=e_dpre) \
        + U * ref["dh1"].abs()
    return dict(ffpre=e_pre, ffact=e_act, ffout=e_out, hout=e_hout, mean=e_mean, rstd=e_rstd, dffout=e_dfo, dpre=e_dpre, dh1=e_dh1)


# ------------------------------------------------------------------------------------------------ the two metrics
def tensor_rel(got, ref):
    """max |err| / max |ref| (0 when both are exactly zero)"""
    ref = ref.to(F64)
    err, top = float((got.to(F64) - ref).abs().max()), float(ref.abs().max())
    return 0.0 if err == 0.0 else err / top if top > 0 else math.inf


def left_out_rows(ref):
    """rows whose fp64 result is not representable as a normal fp32 number: the row's largest magnitude is non-zero and outside
    [2^-126, FLT_MAX]"""
    m = ref.to(F64).abs().amax(dim=1)
    return (m > 0) & ((m < FP32_MIN_NORMAL) | (m > FP32_MAX))


def row_ratio(got, ref, bound, max_left_out=0.02):
    """worst per-row max_f |err| / bound over the rows kept; a row with bound 0 must be exact.  Returns (ratio, rows left out)"""
    ref = ref.to(F64)
    err = (got.to(F64) - ref).abs()
    out = left_out_rows(ref)
    assert int(out.sum()) <= max_left_out * ref.shape[0], f"{int(out.sum())} of {ref.shape[0]} rows left out"
    err, bound = err[~out], bound[~out]
    exact = bound == 0
    assert bool((err[exact] == 0).all()), "an element whose bound is zero is not exactly the reference"
    ratio = torch.where(exact, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    assert not bool(torch.isnan(ratio).any())
    return float(ratio.max()) if ratio.numel() else 0.0, int(out.sum())


# ------------------------------------------------------------------------------------------------ the input families
A_GRID = [(1.0, 1.0, 1.0), (3e-13, 2e7, 1.0), (5e11, 7e-9, 1.0), (1.0, 1.0, 3e-21), (40.0, 0.01, 6e9)]


def f32(t):
    return t.to(F32).to(F64)


def row_exponents(T, g, lo=-30, hi=30):
    """family B: an independent power of two per row, three rows zero (one of them the last row, in a ragged tile)"""
    f = torch.ldexp(torch.ones(T, dtype=F64), torch.randint(lo, hi + 1, (T,), generator=g))
    for z in {min(5, T - 1), T // 2, T - 1}:
        f[z] = 0.0
    return f.view(T, 1)


def mlm_rows(T, g, zero=0.8):
    """the label-row pattern: `zero` of the rows exactly zero"""
    return (torch.rand(T, generator=g, dtype=F64) >= zero).to(F64).view(T, 1)


def ff_params(g, D, scale=0.1):
    r = lambda *s: scale * torch.randn(*s, generator=g, dtype=F64)
    return dict(w1=r(4 * D, D), b1=r(4 * D), w2=r(D, 4 * D), b2=r(D), ff_ln_w=1 + r(D), ff_ln_b=r(D))


FF_FAMILIES = ["A0", "A1", "A2", "A3", "A4", "B", "C12", "C22", "Dw1", "Db1", "Dw1drop", "Etok", "Edy", "Ew2"]


def ff_family(name, T, D, seed=0):
    """(h1, params, dy, drop_p) of a family of the feed-forward tests, as the fp32 values the kernels see, in fp64"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * T + D + 13 * FF_FAMILIES.index(name))
    p = ff_params(g, D)
    h1 = torch.randn(T, D, generator=g, dtype=F64)
    dy = torch.randn(T, D, generator=g, dtype=F64)
    drop_p = 0.0
    if name[0] == "A":
        sx, sw, sg = A_GRID[int(name[1])]
        h1, dy = h1 * sx, dy * sg
        for k in ("w1", "w2"):
            p[k] = p[k] * sw
        p["b1"] = p["b1"] * (sx * sw)
    elif name == "B":
        h1 = h1 * row_exponents(T, g)
        dy = dy * row_exponents(T, g) * mlm_rows(T, g)
    elif name[0] == "C":
        ch = torch.randint(0, D, (T,), generator=g)
        h1[torch.arange(T), ch] *= 2.0 ** int(name[1:])
        dy[torch.arange(T), torch.randint(0, D, (T,), generator=g)] *= 2.0 ** int(name[1:])
    elif name in ("Dw1", "Dw1drop"):
        p["w1"][int(torch.randint(0, 4 * D, (1,), generator=g)), int(torch.randint(0, D, (1,), generator=g))] *= 2.0 ** 10
        drop_p = 0.3 if name == "Dw1drop" else 0.0
    elif name == "Db1":
        p["b1"][int(torch.randint(0, 4 * D, (1,), generator=g))] *= 2.0 ** 16
    elif name == "Etok":
        h1 = torch.zeros_like(h1)
    elif name == "Edy":
        dy = torch.zeros_like(dy)
    elif name == "Ew2":
        p["w2"] = torch.zeros_like(p["w2"])
    return f32(h1), {k: f32(v) for k, v in p.items()}, f32(dy), drop_p
