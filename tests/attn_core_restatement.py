"""Float64 references, per-element error bounds, input families and a plain fp32 restatement of the ALGORITHM of the attention
cores (csrc/xlnet_attn_mfma.hip, csrc/xlnet_attn.hip, csrc/xlnet_attn_long.hip, csrc/mha.hip, csrc/mha_mfma.hip and the
stored-probability backward of include/t4r_hip_attn.h).  No GPU, no HIP library: torch on the CPU only.

The operation (layout here: q, k, v, dout [B, L, n, d]; k_r [2L, n, d]; r_w, r_r [n, d]; scale = d^-1/2)
    XLNet   s_ij = scale ((q_i + r_w) k_j + (q_i + r_r) k_r[j - i + L])        the relative shift of test_xlnet_attention_core
    MHA     s_ij = scale q_i k_j,   keys j <= i only when causal
    p_ij = exp(s_ij - lse_i),  lse_i = log sum_j exp(s_ij),  out_i = sum_j p_ij M_ij v_j
M is the device's dropout keep decision times its factor 1 / (1 - p) as fp32 forms it (ones without dropout).

key_len outside [1, L] (what the kernels do, and what the references here do)
    MHA     klen = max(1, min(L, key_len[b])): keys j >= klen leave the row.  csrc/mha.hip:55, :134, :184;
            csrc/mha_mfma.hip:48, :145; csrc/xlnet_attn_long.hip:350, :391, :426.   key_len <= 0 acts as 1, > L as L.
    XLNet   key j of row i is masked when j >= key_len[b] and j != i, no clamp.  csrc/xlnet_attn.hip:80, :93, :226, :422;
            csrc/xlnet_attn_mfma.hip:154-158, :304-307; csrc/xlnet_attn_long.hip:119, :127, :144.   key_len <= 0: every row
            attends to itself only (p_ii = 1, lse_i = s_ii); key_len >= L: nothing is masked.
    A masked key has probability exactly 0 in the forward and in every gradient: the kernels give it -1e30f (tile padding:
    -INFINITY), and exp(-1e30 - x) is 0 for every finite x, so the reference uses -inf.

Error bounds (u = 2^-24; every line per element, first order; |.| element-wise)
A running-error bound: the same formula in float64 with every term replaced by its absolute value, times a relative factor.
    scores      Sa_ij = scale ((|q_i| + |r_w|) |k_j| + (|q_i| + 2 |r_w| + |r_r|) |k_r[m]|)     (MHA: scale |q_i| |k_j|)
                e_s,ij = K_S u Sa_ij,   K_S = 2 T + 6,  T = 2 d (XLNet: two dots of d terms) or d (MHA).
                2 u per accumulated term (the matrix cores need not round to nearest), the bias add, the sum of the two dots
                and the scale are the + 6.  The matrix-core XLNet kernel forms (q + r_w) k_r + (r_r - r_w) k_r: hence 2 |r_w|.
    exponent    the argument s_ij - m_i (m_i the row maximum) is rounded, and so is its product with log2 e inside __expf:
                eps_ij = e_s,ij + 2 u (|s_ij| + |m_i|) + (2 C_EXP + 1) u
                C_EXP: the one allowance that the source does not give -- the accuracy of the fast __expf / __logf, in ulps
                (2 u) per probability and for lse.
    p           l_i = sum_j w_ij with w_ij = exp(s_ij - m_i) (1 + eps_ij): its relative error is ebar_i = sum_j p_ij eps_ij plus
                the L additions; the online form multiplies o and l by the SAME alpha = exp(m_old - m_new), whose error
                cancels in o / l up to the roundings of the two multiplications per key.
                rho_ij = eps_ij + ebar_i + (3 L + 4) u,     e_p,ij = p_ij rho_ij + 2^-126
                (2^-126: a probability, and every product formed from one, may be flushed to zero below fp32's normal range;
                it is the format's underflow threshold, not a floor for small rows: a probability of 1e-30 is still held to
                its relative bound.  The backward formulas below carry the same term where p'_ij and dS_ij are formed and
                once per term of the last contraction.)
    out         A_out,id = sum_j p_ij M_ij |v_jd|
                e_out,id = sum_j e_p,ij M_ij |v_jd| + (2 L + 4) u A_out,id
    lse         = m + log l.  The alphas do NOT cancel here: every rise of the running maximum (R_i of them in a left-to-right
                pass of the reference scores) costs one __expf and the rounding of its argument, whose sizes sum to at most
                |m_i| + max_j |s_ij|:
                e_lse,i = ebar_i + (3 L + 4) u + R_i (2 C_EXP + 2) u + [R_i > 1] 2 u (|m_i| + max_j |s_ij|)
                          + 2 C_EXP u max(|log l_i|, 1) + u (|m_i| + 2 |log l_i| + |lse_i|)
Backward, dS_ij = scale p_ij (dP_ij M_ij - D_i), the companions carried through its terms:
    dP          dP_ij = dout_i v_j,   e_dP,ij = (2 d + 2) u M_ij sum_h |dout_ih| |v_jh|
    D           D_i = dout_i out_i from the STORED fp32 out:   e_D,i = sum_h |dout_ih| e_out,ih + (2 d + 2) u sum_h |dout_ih| |out_ih|
                (stored-probability backward: D_i = sum_j p_ij M_ij dP_ij,  e_D,i = sum_j p_ij (e_dP,ij + (2 L + 4) u M_ij |dP_ij|))
    p again     p'_ij = __expf(s_ij - lse_i):   rho'_ij = e_s,ij + e_lse,i + 2 u (|s_ij| + |lse_i|) + (2 C_EXP + 1) u
                (stored-probability backward: p is read, rho' = 2 u)
    dS          e_dS,ij = scale (p_ij rho'_ij |dP_ij M_ij - D_i| + p_ij (e_dP,ij + e_D,i) + 3 u p_ij (|dP_ij M_ij| + |D_i|))
                -- in a one-hot row dP - D cancels and only the second, absolute, term is left: that is the cancellation.
    dq_i        sum_j dS_ij (k_j + k_r[m]):     sum_j e_dS,ij (|k_j| + |k_r[m]|) + (2 L + 4) u sum_j |dS_ij| (|k_j| + |k_r[m]|)
    dk_j        sum_i dS_ij (q_i + r_w):        sum_i e_dS,ij (|q_i| + |r_w|) + (2 L + 4) u sum_i |dS_ij| (|q_i| + |r_w|)
    dv_j        sum_i p_ij M_ij dout_i:         sum_i p_ij rho'_ij M_ij |dout_i| + (2 L + 4) u sum_i p_ij M_ij |dout_i|
    dk_r[m]     sum_b sum_{j - i + L = m} dS_ij (q_i + r_r):  the same two terms with |q_i| + 2 |r_w| + |r_r|, and the sum over
                sessions: a nested sum in which no term takes part in more than L + B additions, 2 u each:  (2 (L + B) + 4) u
    dr_w, dr_r  sum_b sum_i sum_j dS_ij k_j (k_r[m]):  nesting depth 2 L + B:  (2 (2 L + B) + 4) u
The bounds are absolute-value based, so NO row is left out of the metric and there is no floor for small rows: an element
whose bound is zero must be exactly the reference.  MULT (below) multiplies the rounding part of every bound (all terms in u);
the underflow terms (2^-126) are a property of the number format and are added unscaled.  How MULT and C_EXP were obtained is
recorded in profiles/attn_core_margins.txt.

Input families (family(name, B, L, n, d, seed, kind)): see FAMILIES and the docstring of each generator.
"""
import math

import torch

F64, F32 = torch.float64, torch.float32
U = 2.0 ** -24
TINY = 2.0 ** -126        # fp32's smallest normal number: a result below it may be flushed to zero
# Every bound is multiplied by MULT: the smallest power of two at which, with C_EXP = 0, the fp32 restatement below (accurate
# exp / log) has its worst error / bound over all families and shapes of tests/test_attn_core_cpu.py at <= 0.5.  Fixed from the
# CPU run alone (worst at MULT = 1: 0.225, dv of the backward that reads the probabilities, family U; the recomputing paths
# 0.137, lse, family P of the MHA core), before any kernel was measured.
MULT = 0.5
# ulps (2 u) allowed to the fast __expf / __logf per probability and for lse; the smallest integer that puts the worst kernel of
# the unit-scale family at <= 0.5 of the bound on an MI355X: every kernel group is there without an allowance
# (profiles/attn_core_margins.txt; tests/test_attn_core_gpu.py prints the figure for family U on every run)
C_EXP = 0

GRAD_NAMES = {"xlnet": ("dq", "dk", "dv", "dkr", "drw", "drr"), "mha": ("dq", "dk", "dv")}


def f32(t):
    return t.to(F32).to(F64)


def heads(t):
    """[B, L, n, d] -> [B, n, L, d]"""
    return t.permute(0, 2, 1, 3)


# ------------------------------------------------------------------------------------------------ masks
def _ij(L):
    return torch.arange(L)[:, None], torch.arange(L)[None, :]


def xlnet_dead(B, L, key_len):
    """[B, 1, L, L] bool: key j of row i is masked (csrc/xlnet_attn.hip:93: j >= klen && j != i, no clamp)"""
    if key_len is None:
        return torch.zeros(B, 1, L, L, dtype=torch.bool)
    i, j = _ij(L)
    return ((j[None] >= key_len.long().view(B, 1, 1)) & (j != i)[None])[:, None]


def mha_dead(B, L, causal, key_len, clamp=True, strict=False):
    """[B, 1, L, L] bool: key j is outside row i (csrc/mha.hip:55-56: j >= min(causal ? i + 1 : L, clamp(key_len, 1, L))).
    clamp=False, strict=True are planted faults 7 and 8 of the fp32 restatement"""
    i, j = _ij(L)
    dead = torch.zeros(B, 1, L, L, dtype=torch.bool)
    if causal:
        dead = dead | ((j >= i) if strict else (j > i))[None, None]
    if key_len is not None:
        kl = key_len.long()
        if clamp:
            kl = kl.clamp(1, L)
        dead = dead | (j[None] >= kl.view(B, 1, 1))[:, None]
    return dead


def shift_index(B, n, L):
    i, j = _ij(L)
    return (j - i + L).expand(B, n, L, L)


# ------------------------------------------------------------------------------------------------ float64 references
def xlnet_scores(q, k, kr, rw, rr):
    """scaled scores [B, n, L, L] in the dtype of the inputs"""
    B, L, n, d = q.shape
    ac = torch.einsum("bind,bjnd->bnij", q + rw, k)
    raw = torch.einsum("bind,pnd->bnip", q + rr, kr)
    return (ac + torch.gather(raw, 3, shift_index(B, n, L))) / math.sqrt(d)


def mha_scores(q, k):
    return torch.einsum("bind,bjnd->bnij", q, k) / math.sqrt(q.shape[-1])


def _core(s, v, dead, mask):
    s = s.masked_fill(dead, float("-inf"))
    lse = torch.logsumexp(s, 3)
    prob = torch.exp(s - lse[..., None])
    pm = prob if mask is None else prob * mask
    return torch.einsum("bnij,bjnd->bind", pm, v), lse, prob


def xlnet_core(q, k, v, kr, rw, rr, key_len=None, mask=None):
    """-> out [B, L, n, d], lse [B, n, L], prob [B, n, L, L] (before dropout).  mask [B, n, L, L]: keep times factor"""
    B, L = q.shape[:2]
    return _core(xlnet_scores(q, k, kr, rw, rr), v, xlnet_dead(B, L, key_len), mask)


def mha_core(q, k, v, causal, key_len=None, mask=None):
    B, L = q.shape[:2]
    return _core(mha_scores(q, k), v, mha_dead(B, L, causal, key_len), mask)


def reference(kind, x, causal=False, key_len=None, mask=None):
    """float64 forward and autograd of one case.  x: dict of q, k, v, dout (XLNet: kr, rw, rr).  -> dict out, lse, prob, d*"""
    names = ("q", "k", "v", "kr", "rw", "rr") if kind == "xlnet" else ("q", "k", "v")
    leaf = [x[nm].to(F64).clone().requires_grad_() for nm in names]
    if kind == "xlnet":
        out, lse, prob = xlnet_core(*leaf, key_len=key_len, mask=mask)
    else:
        out, lse, prob = mha_core(*leaf, causal, key_len=key_len, mask=mask)
    grads = torch.autograd.grad(out, leaf, x["dout"].to(F64))
    ref = dict(out=out.detach(), lse=lse.detach(), prob=prob.detach())
    ref.update({"d" + nm: g for nm, g in zip(names, grads)})
    return ref


# ------------------------------------------------------------------------------------------------ the bounds
def _scatter_shift(X, Y, L):
    """sum_b sum_{j - i + L = m} X[b, n, i, j] Y[b, n, i, d] -> [2L, n, d]"""
    B, n = X.shape[:2]
    Z = torch.zeros(B, n, L, 2 * L, dtype=X.dtype).scatter_(3, shift_index(B, n, L), X)
    return torch.einsum("bnim,bnid->mnd", Z, Y)


def bounds(kind, x, ref, causal=False, key_len=None, mask=None, c_exp=None, mult=None, p_given=False):
    """per-element bounds (module docstring) for out, lse, prob and every gradient, in the layout of `reference`.
    p_given: the stored-probability backward (p is read from memory, D_i from p and dP).
    Every formula is linear in (u, 2^-126): the rounding part is evaluated with the underflow threshold at 0 and multiplied by
    MULT, the underflow part with u = 0 and NOT multiplied -- it is a property of the format, not of the calibration"""
    c = C_EXP if c_exp is None else c_exp
    mult = MULT if mult is None else mult
    rnd = _bounds(kind, x, ref, causal, key_len, mask, c, p_given, U, 0.0)
    flush = _bounds(kind, x, ref, causal, key_len, mask, c, p_given, 0.0, TINY)
    return {nm: mult * rnd[nm] + flush[nm] for nm in rnd}


def _bounds(kind, x, ref, causal, key_len, mask, c, p_given, U, TINY):
    q, k, v, g = (heads(x[nm].to(F64)) for nm in ("q", "k", "v", "dout"))               # [B, n, L, d]
    B, n, L, d = q.shape
    scale = 1.0 / math.sqrt(d)
    M = torch.ones(B, n, L, L, dtype=F64) if mask is None else mask.to(F64).abs()
    mm = lambda a, b: torch.einsum("bnih,bnjh->bnij", a, b)
    if kind == "xlnet":
        kr = x["kr"].to(F64).permute(1, 0, 2)                                            # [n, 2L, d]
        rw, rr = x["rw"].to(F64)[None, :, None, :], x["rr"].to(F64)[None, :, None, :]
        idx = shift_index(B, n, L)
        mr = lambda a: torch.gather(torch.einsum("bnih,nmh->bnim", a, kr.abs()), 3, idx)
        qk, qkr = q.abs() + rw.abs(), q.abs() + 2 * rw.abs() + rr.abs()
        Sa = scale * (mm(qk, k.abs()) + mr(qkr))
        s = xlnet_scores(*(x[nm].to(F64) for nm in ("q", "k", "kr", "rw", "rr")))
        dead = xlnet_dead(B, L, key_len).expand(B, n, L, L)
        T = 2 * d
    else:
        Sa = scale * mm(q.abs(), k.abs())
        s = mha_scores(x["q"].to(F64), x["k"].to(F64))
        dead = mha_dead(B, L, causal, key_len).expand(B, n, L, L)
        qk = q.abs()
        T = d
    zero = torch.zeros_like(s)
    live = lambda t: torch.where(dead, zero, t)
    p, lse = ref["prob"], ref["lse"][..., None]                                          # [B, n, L, L], [B, n, L, 1]
    e_s = live((2 * T + 6) * U * Sa)
    sabs = live(s.abs())
    m = s.masked_fill(dead, float("-inf")).amax(3, keepdim=True)
    smax = sabs.amax(3, keepdim=True)
    eps = live(e_s + 2 * U * (sabs + m.abs()) + (2 * c + 1) * U)
    ebar = (p * eps).sum(3, keepdim=True)
    rho = eps + ebar + (3 * L + 4) * U
    e_p = live(p * rho + TINY)
    pM = p * M
    e_out = torch.einsum("bnij,bnjh->bnih", e_p * M, v.abs()) + (2 * L + 4) * U * torch.einsum("bnij,bnjh->bnih", pM, v.abs())
    # rises of the running maximum in a left-to-right pass
    run = torch.cummax(s.masked_fill(dead, float("-inf")), 3).values
    rises = 1 + (run[..., 1:] > run[..., :-1]).sum(3, keepdim=True).to(F64)
    logl = lse - m
    e_lse = (ebar + (3 * L + 4) * U + rises * (2 * c + 2) * U + (rises > 1).to(F64) * 2 * U * (m.abs() + smax)
             + 2 * c * U * logl.abs().clamp_min(1.0) + U * (m.abs() + 2 * logl.abs() + lse.abs()))
    # backward
    out = heads(ref["out"])
    dP = mm(g, v)
    dPM = dP * (M if mask is None else mask.to(F64))
    e_dP = (2 * d + 2) * U * M * mm(g.abs(), v.abs())
    D = (g * out).sum(3, keepdim=True)
    if p_given:
        e_D = (p * (e_dP + (2 * L + 4) * U * dPM.abs())).sum(3, keepdim=True)
        e_p2 = live(2 * U * p + TINY)
    else:
        e_D = (g.abs() * e_out).sum(3, keepdim=True) + (2 * d + 2) * U * (g.abs() * out.abs()).sum(3, keepdim=True)
        e_p2 = live(p * (e_s + e_lse + 2 * U * (sabs + lse.abs()) + (2 * c + 1) * U) + TINY)
    dS = scale * p * (dPM - D)
    e_dS = scale * (e_p2 * (dPM - D).abs() + p * (e_dP + e_D) + 3 * U * p * (dPM.abs() + D.abs()))
    e_dS = torch.where((dPM == 0) & (D == 0) & (e_D == 0), zero, e_dS + TINY)
    acc = (2 * L + 4) * U
    ctr = lambda a, b: torch.einsum("bnij,bnjh->bnih", a, b)            # over keys
    ctr_i = lambda a, b: torch.einsum("bnij,bnih->bnjh", a, b)          # over queries
    bd = dict(out=e_out, lse=e_lse[..., 0], prob=e_p)
    e_dq = ctr(e_dS, k.abs()) + acc * ctr(dS.abs(), k.abs())
    bd["dk"] = ctr_i(e_dS, qk) + acc * ctr_i(dS.abs(), qk)
    bd["dv"] = ctr_i(e_p2 * M, g.abs()) + acc * ctr_i(pM, g.abs())
    if kind == "xlnet":
        krg = lambda X: torch.einsum("bnim,nmh->bnih", torch.zeros(B, n, L, 2 * L, dtype=F64).scatter_(3, idx, X), kr.abs())
        e_dq = e_dq + krg(e_dS) + acc * krg(dS.abs())
        bd["dkr"] = (_scatter_shift(e_dS, qkr, L) + (2 * (L + B) + 4) * U * _scatter_shift(dS.abs(), qkr, L))
        deep = (2 * (2 * L + B) + 4) * U
        bd["drw"] = (ctr(e_dS, k.abs()) + deep * ctr(dS.abs(), k.abs())).sum((0, 2))
        bd["drr"] = (krg(e_dS) + deep * krg(dS.abs())).sum((0, 2))
    bd["dq"] = e_dq
    # a product below fp32's normal range may be flushed: TINY per term of the last contraction (none where every term is 0)
    terms = dict(dq=L, dk=L, dv=L, dkr=L * B, drw=L * L * B, drr=L * L * B)
    for nm in terms:
        if nm in bd:
            bd[nm] = torch.where(bd[nm] > 0, bd[nm] + terms[nm] * TINY, bd[nm])
    for nm in ("out", "dq", "dk", "dv"):
        bd[nm] = bd[nm].permute(0, 2, 1, 3)                                               # back to [B, L, n, d]
    return bd


def ratio(got, ref, bound):
    """worst |err| / bound over EVERY element; an element whose bound is zero must be exact (then 0), else inf.
    A non-finite value gives inf"""
    got, ref = got.to(F64).reshape(ref.shape), ref.to(F64)
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    r = torch.where((bound == 0) & (err > 0), torch.full_like(err, math.inf), r)
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------ the input families
FAMILIES = ("U", "P", "A+", "A-", "O+", "O-", "E", "Z1", "Z2")       # M is key_len on top of U and O- (mask_edges)
O_TARGET = {"O+": 95.0, "O-": -110.0}


def mask_edges(L):
    """family M: key_len of five sessions -- 0 (MHA: clamps to 1; XLNet: diagonal only), 1, a mid value, L and L + 5
    (unmasked).  Catches the clamp, the diagonal exemption, -1e30f beside real scores near -110, NaN from an empty row"""
    return torch.tensor([0, 1, max(1, L // 2), L, L + 5], dtype=torch.int32)


def _scores_of(kind, x):
    return xlnet_scores(x["q"], x["k"], x["kr"], x["rw"], x["rr"]) if kind == "xlnet" else mha_scores(x["q"], x["k"])


def family(name, B, L, n, d, seed=0, kind="xlnet"):
    """dict of q, k, v, dout [B, L, n, d], kr [2L, n, d], rw, rr [n, d]: fp32 values held in float64.
    U   unit      randn, biases 0.5 randn, as tests/test_kernels_gpu.py.  Baseline, indexing, small rows beside large ones.
    P   peaked    keys of norm sqrt(d): signed axes for the first 2 d of them, random directions after; query i copies key
                  t_i <= i (visible under the causal bound); q scaled so that max |s| = 70.  One-hot softmax, the backward's
                  cancellation, lse accuracy.
    A+/A- ascending / descending   k_j = c (j + 1) e, q_i = e' with scale e e' = 1, c = +-min(3, 60 / L); noise 1e-3; k_r and the
                  biases 1e-3.  The running maximum rises at every key (A+) or never after the first (A-).
    O+/O- offset  q_i = a e + noise, k_j = +-a e + noise with scale a^2 = |target|, noise sized so that every score of a row is
                  within +-2 of +95 / -110.  exp(s) overflows / the sum of exp(s) underflows without the maximum.
    E   equal     every key of a (session, head) identical, k_r and the biases zero: p = 1 / L (causal 1 / (i + 1)) exactly,
                  out = mean of v, dq = 0.
    Z1  zeros     v = 0 and every third row of dout zero: out, dq, dk, dkr, drw, drr exactly zero, no NaN.
    Z2  zeros     q = 0 (MHA: uniform rows), no NaN."""
    g = torch.Generator().manual_seed(100003 * seed + 1009 * B + 31 * L + 7 * n + d + 13 * FAMILIES.index(name)
                                      + (0 if kind == "xlnet" else 5))
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    x = dict(q=r(B, L, n, d), k=r(B, L, n, d), v=r(B, L, n, d), dout=r(B, L, n, d), kr=r(2 * L, n, d), rw=0.5 * r(n, d),
             rr=0.5 * r(n, d))
    scale = 1.0 / math.sqrt(d)
    if name == "P":
        k = r(B, L, n, d)
        k = k / k.norm(dim=-1, keepdim=True)
        axes = min(L, 2 * d)
        ax = torch.zeros(axes, d, dtype=F64)
        ax[torch.arange(axes), torch.arange(axes) % d] = 1.0 - 2.0 * ((torch.arange(axes) // d) % 2).to(F64)
        k[:, :axes] = ax[:, None, :] + 0.03 * r(B, axes, n, d)
        k = k * math.sqrt(d)
        t = (torch.rand(B, L, n, generator=g) * (torch.arange(L) + 1).view(1, L, 1)).long().clamp_max(L - 1)   # t_i <= i
        q = torch.gather(k, 1, t[..., None].expand(B, L, n, d)) + 0.05 * r(B, L, n, d)
        x.update(q=q, k=k, kr=0.1 * x["kr"], rw=0.1 * x["rw"], rr=0.1 * x["rr"])
        for _ in range(3):
            x["q"] = f32(x["q"] * (70.0 / float(_scores_of(kind, {z: f32(t_) for z, t_ in x.items()}).abs().max())))
    elif name in ("A+", "A-"):
        c = (1.0 if name == "A+" else -1.0) * min(3.0, 60.0 / L)
        e = r(n, d).abs() + 0.5
        e = e / e.norm(dim=-1, keepdim=True)
        j1 = (torch.arange(L, dtype=F64) + 1).view(1, L, 1, 1)
        x["k"] = c * j1 * e + 1e-3 * r(B, L, n, d)
        x["q"] = (e / scale) * (1 + 1e-3 * r(B, L, n, d))
        x.update(kr=1e-3 * x["kr"], rw=1e-3 * x["rw"], rr=1e-3 * x["rr"])
    elif name in ("O+", "O-"):
        tgt = O_TARGET[name]
        e = r(n, d)
        e = e / e.norm(dim=-1, keepdim=True)
        a = math.sqrt(abs(tgt) / scale)
        nq, nk = r(B, L, n, d), r(B, L, n, d)
        x.update(kr=0.01 * x["kr"], rw=0.01 * x["rw"], rr=0.01 * x["rr"])
        f = 0.05
        for _ in range(4):
            x["q"], x["k"] = a * e + f * nq, math.copysign(a, tgt) * e + f * nk
            dev = float((_scores_of(kind, {z: f32(t_) for z, t_ in x.items()}) - tgt).abs().max())
            f = f * 1.7 / dev if dev > 1.9 or dev < 1.2 else f
    elif name == "E":
        x["k"] = r(B, 1, n, d).expand(B, L, n, d).clone()
        x.update(kr=torch.zeros(2 * L, n, d, dtype=F64), rw=torch.zeros(n, d, dtype=F64), rr=torch.zeros(n, d, dtype=F64))
    elif name == "Z1":
        x["v"] = torch.zeros(B, L, n, d, dtype=F64)
        x["dout"][:, ::3] = 0.0
    elif name == "Z2":
        x["q"] = torch.zeros(B, L, n, d, dtype=F64)
    return {z: f32(t_).contiguous() for z, t_ in x.items()}


# ---- what a family must do before it is used on the GPU (tests/test_attn_core_cpu.py)
def running_max_changes(s, dead):
    """[B, n, L]: at how many keys of its row the running maximum of a left-to-right pass changes (the first key counts)"""
    run = torch.cummax(s.masked_fill(dead, float("-inf")), 3).values
    return 1 + (run[..., 1:] > run[..., :-1]).sum(3)


def peaked_fraction(prob):
    """fraction of rows whose largest probability is at least 0.99"""
    return float((prob.amax(3) >= 0.99).double().mean())


def naive_exp_fails(s, dead, sign):
    """fp32 exp(s) without the maximum: every live one inf (sign > 0) / every row's fp32 sum exactly 0 (sign < 0)"""
    e = torch.exp(s.to(F32))
    if sign > 0:
        return bool(torch.isinf(e[~dead]).all())
    return bool((torch.where(dead, torch.zeros_like(e), e).sum(3) == 0).all())


# ------------------------------------------------------------------------------------------------ the fp32 restatement
FAULTS = {1: "no maximum subtraction", 2: "o not multiplied by alpha when the maximum rises",
          3: "lse written with the maximum of the previous block", 4: "D_i from the un-normalised accumulator",
          5: "lse rounded to fp16 before the backward reads it", 6: "masked keys at -100 instead of -1e30 (XLNet)",
          7: "no key_len clamp in MHA", 8: "causal bound j < i instead of j <= i", 9: "the diagonal not exempted from the XLNet mask"}


def restated(kind, x, causal=False, key_len=None, mask=None, block=16, fault=0, prob=None):
    """The kernels' ALGORITHM in fp32 with accurate exp / log: blockwise online softmax over `block` keys with running m, l and
    alpha, lse = m + log l, and a backward that recomputes p from lse with D from the stored out.  fault: one of FAULTS.
    prob: the backward reads these probabilities (rounded to fp32) instead, with D_i = sum_j p_ij M_ij dP_ij.
    -> the dict of `reference` (without prob)"""
    X = {z: t_.to(F32) for z, t_ in x.items()}
    q, k, v, g = (heads(X[nm]) for nm in ("q", "k", "v", "dout"))
    B, n, L, d = q.shape
    scale = torch.tensor(1.0 / math.sqrt(d), dtype=F32)
    M = torch.ones(B, n, L, L, dtype=F32) if mask is None else mask.to(F32)
    NEG = torch.tensor(float("-inf"), dtype=F32)
    if kind == "xlnet":
        s = xlnet_scores(X["q"], X["k"], X["kr"], X["rw"], X["rr"])
        dead = xlnet_dead(B, L, key_len)
        if fault == 9 and key_len is not None:
            dead = (_ij(L)[1][None] >= key_len.long().view(B, 1, 1))[:, None]
        s = torch.where(dead.expand_as(s), torch.tensor(-100.0 if fault == 6 else -1e30, dtype=F32), s)
        off = torch.zeros_like(dead).expand_as(s)
    else:
        s = mha_scores(X["q"], X["k"])
        off = mha_dead(B, L, causal, key_len, clamp=fault != 7, strict=fault == 8).expand_as(s)
    m = torch.full((B, n, L), float("-inf"), dtype=F32)
    m_prev = m.clone()
    l = torch.zeros(B, n, L, dtype=F32)
    o = torch.zeros(B, n, L, d, dtype=F32)
    for j0 in range(0, L, block):
        j1 = min(L, j0 + block)
        sb, ob = s[..., j0:j1], off[..., j0:j1]
        bm = torch.where(ob, NEG, sb).amax(3)
        mn = torch.zeros_like(m) if fault == 1 else torch.maximum(m, bm)
        alpha = torch.where(torch.isinf(mn) & (mn < 0), torch.ones_like(m), torch.exp(m - mn))
        if fault == 1:
            alpha = torch.ones_like(m)
        pj = torch.where(ob, torch.zeros_like(sb), torch.exp(sb - mn[..., None]))
        l = l * alpha + pj.sum(3)
        o = (o if fault == 2 else o * alpha[..., None]) + torch.einsum("bnij,bnjh->bnih", pj * M[..., j0:j1], v[:, :, j0:j1])
        m_prev, m = m, mn
    out = o / l[..., None]
    lse = (m_prev if fault == 3 and L > block else m) + torch.log(l)
    res = dict(out=out.permute(0, 2, 1, 3), lse=lse)
    # backward
    lse_b = lse.to(torch.float16).to(F32) if fault == 5 else lse
    D = (g * (o if fault == 4 else out)).sum(3, keepdim=True)
    p = torch.where(off, torch.zeros_like(s), torch.exp(s - lse_b[..., None]))
    dP = torch.einsum("bnih,bnjh->bnij", g, v) * M
    if prob is not None:
        p = prob.to(F32)
        D = (p * dP).sum(3, keepdim=True)
    dS = p * (dP - D) * scale
    ctr = lambda a, b: torch.einsum("bnij,bnjh->bnih", a, b)
    dq = ctr(dS, k)
    res["dv"] = torch.einsum("bnij,bnih->bnjh", p * M, g).permute(0, 2, 1, 3)
    if kind == "xlnet":
        kr = X["kr"].permute(1, 0, 2)
        Z = torch.zeros(B, n, L, 2 * L, dtype=F32).scatter_(3, shift_index(B, n, L), dS)
        dqb = torch.einsum("bnim,nmh->bnih", Z, kr)
        res["dk"] = torch.einsum("bnij,bnih->bnjh", dS, q + X["rw"][None, :, None, :]).permute(0, 2, 1, 3)
        res["dkr"] = torch.einsum("bnim,bnih->mnh", Z, q + X["rr"][None, :, None, :])
        res["drw"], res["drr"] = dq.sum((0, 2)), dqb.sum((0, 2))
        dq = dq + dqb
    else:
        res["dk"] = torch.einsum("bnij,bnih->bnjh", dS, q).permute(0, 2, 1, 3)
    res["dq"] = dq.permute(0, 2, 1, 3)
    return res


def worst_ratios(kind, x, got, causal=False, key_len=None, mask=None, ref=None, bd=None, **kw):
    """{output name: worst error / bound} of `got` (a dict in the layout of `reference`) for one case"""
    ref = reference(kind, x, causal, key_len, mask) if ref is None else ref
    bd = bounds(kind, x, ref, causal, key_len, mask, **kw) if bd is None else bd
    return {nm: ratio(got[nm], ref[nm], bd[nm]) for nm in got if nm in bd}


# ------------------------------------------------------------------------------------------------ the shapes of both suites
# (B, L, D, n): the smallest that reach each kernel and its edges
XLNET_SHAPES = [(3, 20, 64, 4), (2, 32, 64, 2), (2, 1, 32, 2), (2, 17, 16, 1),              # one-wave matrix-core kernels
                (2, 20, 16, 2), (2, 33, 32, 2), (2, 64, 32, 2),                              # VALU / LDS kernels
                (2, 65, 32, 2), (1, 130, 16, 1), (2, 20, 48, 2), (2, 9, 20, 2), (2, 20, 320, 2)]   # general kernels
XLNET_STRIDE_SHAPES = [(1030, 5, 32, 1), (1030, 5, 16, 1)]                                   # sessions past the block cap: U, A+
# (B, L, D, n, causal)
MHA_SHAPES = [(2, 20, 32, 2, True), (2, 20, 32, 2, False), (2, 33, 64, 1, True), (2, 128, 32, 1, False), (2, 7, 64, 1, True),
              (2, 129, 64, 2, True), (2, 30, 100, 4, False), (2, 20, 48, 2, True)]           # the last three: general kernels
