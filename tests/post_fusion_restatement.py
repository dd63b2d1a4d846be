"""float64 restatement of the post-context fusion (csrc/post_fusion.hip, include/t4r_hip_postfusion.h), forward and gradients, the
error bounds its tests use, and planted faults that those bounds have to catch.  Host tensors only.

Symbols: seq [B, L, D], ctx [B, L, C] (sequence-level) or [B, C] (session-level: row b serves every position of session b),
W [D, C], b [D]; p = b + ctx W^T; mode "mul": out = seq (1 + p), "sum": out = seq + p, "concat": out = seq | ctx.

Bounds, EPS = 2^-24 (one fp32 rounding), A = |b| + |ctx| |W|^T, valid for ANY summation order of fp32 products and sums (a sum
of n terms, fused or not, is within (n - 1 + roundings of the terms) EPS of the exact sum of the magnitudes, to first order; the
constants below leave a few EPS for the second-order terms at the sizes tested):
    out, mul    (C + 4) EPS |seq| (1 + A)      p: C roundings; 1 + p: one; the product: one
    out, sum    (C + 3) EPS (|seq| + A)
    dseq, mul   (C + 4) EPS |dout| (1 + A)     dseq, sum and everything of concat at a sequence-level context: exact
    d_w         (T + 3) EPS sum_t |g| |ctx|    g = dout seq (mul: one rounding more per term) or dout
    d_b         (T + 3) EPS sum_t |g|
    dctx        (D + 3) EPS sum_d |g| |W|      session-level: (L D + 3) EPS sum_{l, d} |g| |W|
    dctx of concat at a session-level context: a sum of L fp32 terms, (L + 3) EPS sum_l |dout| (exact for L = 1)."""
import torch

EPS = 2.0 ** -24
MODES = ("mul", "sum", "concat")
MODE_ID = {"mul": 0, "sum": 1, "concat": 2}
AGGREGATION = {"mul": "elementwise-mul", "sum": "elementwise-sum", "concat": "concat"}
FAULTS = ("no_one_plus", "no_bias", "c_truncated", "session_row_mod", "dw_overwritten", "dctx_last_token", "g_of_sum")


def expand(ctx, L):
    """[B, L, C] float64 view of the context: a 2-D context repeated over the L positions"""
    ctx = ctx.double()
    return ctx.unsqueeze(1).expand(-1, L, -1) if ctx.dim() == 2 else ctx


def project(ctx, L, W, b, fault=None):
    """p [B, L, D] float64 and A = |b| + |ctx| |W|^T"""
    x = expand(ctx, L)
    W, b = W.double(), b.double()
    A = b.abs() + x.abs() @ W.abs().t()
    if fault == "session_row_mod" and ctx.dim() == 2:
        B = ctx.shape[0]
        t = torch.arange(B * L)
        x = ctx.double()[(t % L) % B].view(B, L, -1)           # row t % L instead of t / L
    if fault == "c_truncated":
        k = (W.shape[1] - 1) // 4 * 4                           # the contraction stops at a multiple of 4 below C
        x, W = x[..., :k], W[:, :k]
    p = x @ W.t()
    if fault != "no_bias":
        p = p + b
    return p, A


def forward(seq, ctx, W, b, mode, fault=None):
    """-> (out float64, bound); bound is None where the result is a bit copy (concat)"""
    seq = seq.double()
    L = seq.shape[1]
    if mode == "concat":
        return torch.cat([seq, expand(ctx, L)], dim=-1), None
    C = ctx.shape[-1]
    p, A = project(ctx, L, W, b, fault)
    if mode == "mul":
        out = seq * p if fault == "no_one_plus" else seq * (1.0 + p)
        return out, (C + 4) * EPS * seq.abs() * (1.0 + A)
    return seq + p, (C + 3) * EPS * (seq.abs() + A)


def gradients(dout, seq, ctx, W, b, mode, d_w0=None, d_b0=None, fault=None):
    """-> dict name -> (value float64, bound or None = exact) for dseq, dctx and, for the projected modes, d_w and d_b (ADDED to
    the start values d_w0, d_b0 where given; the bound covers the one extra add)"""
    dout = dout.double()
    B, L = dout.shape[:2]
    T = B * L
    x = expand(ctx, L)
    C = ctx.shape[-1]
    session = ctx.dim() == 2
    if mode == "concat":
        D = dout.shape[-1] - C
        dctx = dout[..., D:]
        if not session:
            return {"dseq": (dout[..., :D], None), "dctx": (dctx, None)}
        n = L - 1 if fault == "dctx_last_token" else L
        return {"dseq": (dout[..., :D], None),
                "dctx": (dctx[:, :n].sum(1), (L + 3) * EPS * dctx.abs().sum(1) if L > 1 else None)}
    seq = seq.double()
    D = dout.shape[-1]
    Wd = W.double()
    p, A = project(ctx, L, W, b)
    if mode == "mul":
        dseq, dseq_bound = dout * (1.0 + p), (C + 4) * EPS * dout.abs() * (1.0 + A)
        g = dout if fault == "g_of_sum" else dout * seq
        g_abs = (dout * seq).abs()
    else:
        dseq, dseq_bound, g, g_abs = dout, None, dout, dout.abs()
    g2, x2 = g.reshape(T, D), x.reshape(T, C)
    d_w, d_b = g2.t() @ x2, g2.sum(0)
    bw = (T + 3) * EPS * (g_abs.reshape(T, D).t() @ x2.abs())
    bb = (T + 3) * EPS * g_abs.reshape(T, D).sum(0)
    if d_w0 is not None and fault != "dw_overwritten":
        d_w = d_w + d_w0.double()
        bw = bw + EPS * d_w.abs()
    if d_b0 is not None:
        d_b = d_b + d_b0.double()
        bb = bb + EPS * d_b.abs()
    dctx = g @ Wd
    bc = g_abs @ Wd.abs()
    if session:
        n = L - 1 if fault == "dctx_last_token" else L
        dctx, bc = dctx[:, :n].sum(1), (L * D + 3) * EPS * bc.sum(1)
    else:
        bc = (D + 3) * EPS * bc
    return {"dseq": (dseq, dseq_bound), "dctx": (dctx, bc), "d_w": (d_w, bw), "d_b": (d_b, bb)}


def ratio(got, want, bound):
    """worst error / bound of an fp32 result against its float64 restatement (0 where both error and bound are 0); an exact
    quantity (bound None) gives 0.0 for equal values and inf otherwise"""
    err = (got.double() - want).abs()
    if bound is None:
        return 0.0 if bool((err == 0).all()) else float("inf")
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


def make_case(B, L, D, C, session, scale=1.0, seed=0):
    """inputs of one case: seq, ctx, dout (for the projected modes; concat's is wider: dout_cat), W and b as torch.nn.Linear
    draws them, and non-zero start values of d_w and d_b"""
    g = torch.Generator().manual_seed(seed * 7919 + B * 1000003 + L * 10007 + D * 101 + C * 3 + int(session))
    k = 1.0 / C ** 0.5
    return dict(seq=torch.randn((B, L, D), generator=g) * scale,
                ctx=torch.randn((B, C) if session else (B, L, C), generator=g) * scale,
                dout=torch.randn((B, L, D), generator=g) * scale,
                dout_cat=torch.randn((B, L, D + C), generator=g) * scale,
                W=(torch.rand((D, C), generator=g) * 2 - 1) * k, b=(torch.rand((D,), generator=g) * 2 - 1) * k,
                d_w0=torch.randn((D, C), generator=g), d_b0=torch.randn((D,), generator=g))


def torch_chain(k, mode, accumulate=False):
    """the reference's chain in fp32 torch on the host (F.linear, then * or +, or cat, then autograd) -> (out, grads dict)"""
    seq, ctx = k["seq"].clone().requires_grad_(), k["ctx"].clone().requires_grad_()
    W, b = k["W"].clone().requires_grad_(), k["b"].clone().requires_grad_()
    L = seq.shape[1]
    x = ctx.unsqueeze(1).repeat(1, L, 1) if ctx.dim() == 2 else ctx
    if mode == "concat":
        out = torch.cat([seq, x], dim=-1)
        out.backward(k["dout_cat"])
        return out.detach(), {"dseq": seq.grad, "dctx": ctx.grad}
    p = torch.nn.functional.linear(x, W, b)
    out = torch.multiply(seq, 1.0 + p) if mode == "mul" else seq + p
    if accumulate:
        W.grad, b.grad = k["d_w0"].clone(), k["d_b0"].clone()
    out.backward(k["dout"])
    return out.detach(), {"dseq": seq.grad, "dctx": ctx.grad, "d_w": W.grad, "d_b": b.grad}
