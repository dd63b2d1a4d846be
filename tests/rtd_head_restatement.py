"""float64 restatement of the replaced-token-detection head (csrc/rtd_head.hip, include/t4r_hip_rtd.h) and the per-element
error bounds its fp32 evaluations are held to (tests/test_rtd_cpu.py, tests/test_rtd_gpu.py).  Plain torch on the CPU.

    a = b1 + x W1^T      h = act(a)      z = b2 + h w2      row = max(z, 0) - z y + log1p(exp(-|z|))
    n = sum active       loss = (1 / n) sum_active row      (n = 0: loss 0, every gradient 0)
    dz = active (g / n) (sigmoid(z) - y)      da = dz w2 * act'(a)      dx = da W1
    dW1 = da^T x      db1 = sum_t da      dw2 = sum_t dz h      db2 = sum_t dz

Bounds.  u = 2^-24.  An fp32 chain of n multiply-adds carries at most (n + 2) u sum |terms| (the standard accumulation bound,
any order, with or without fused multiply-adds; + 2 for the seed and a final operation).  The bounds compose through the
chain with the Lipschitz constants of the functions between (erf-GELU: 1.13 for act, 0.8 for act'; the logistic loss: 1;
sigmoid: 1/4), sums over the T tokens have their own length factor T + 3 (T adds in any order, the add into a pre-filled
gradient, the product), and every transcendental (erf, exp, log1p) has a budget of K_ULP ulp of its result on top of the
roundings of the arithmetic around it.  ReLU's derivative jumps at 0: where |a| is within a's own bound of 0 the whole
derivative is allowed to differ.

K_ULP was fixed from the measured worst error / bound ratio with K = 0 on the MI355X (profiles/rtd_head_margins.txt): the rule
is the smallest K that keeps the worst ratio <= 0.5, and with K = 0 the worst ratio over the test inputs is 0.026 (d W1 at
T = 1, D = 16), so K_ULP = 0 -- the roundings counted around each transcendental already cover the device's erf / exp / log1p.
"""
import math

import torch

U = 2.0 ** -24
K_ULP = 0
GELU, RELU = 0, 1
F64 = torch.float64


def _d(t):
    return None if t is None else t.detach().cpu().to(F64)


def act_of(a, act):
    return torch.relu(a) if act == RELU else 0.5 * a * (1.0 + torch.erf(a / math.sqrt(2.0)))


def act_grad_of(a, act):
    if act == RELU:
        return (a > 0).to(a.dtype)
    return 0.5 * (1.0 + torch.erf(a / math.sqrt(2.0))) + a * torch.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)


def forward(x, active, label, W1, b1, w2, b2, act):
    """x [T, D]; active, label bool [T] or None -> dict of float64 tensors: a, h [T, D]; z [T]; and with labels row [T]
    (every token's, inactive ones too), on [T] (0 / 1), n (int), loss"""
    x, W1, b1, w2, b2 = _d(x), _d(W1), _d(b1).view(-1), _d(w2).view(-1), _d(b2).view(-1)
    a = b1[None, :] + x @ W1.t()
    h = act_of(a, act)
    z = b2[0] + h @ w2
    out = {"a": a, "h": h, "z": z}
    if label is None:
        return out
    y = label.detach().cpu().to(F64).view(-1)
    on = torch.ones_like(z) if active is None else active.detach().cpu().to(F64).view(-1)
    row = torch.clamp(z, min=0) - z * y + torch.log1p(torch.exp(-z.abs()))
    n = int(on.sum())
    out.update(y=y, on=on, row=row, n=n, loss=(row * on).sum() / n if n > 0 else torch.zeros((), dtype=F64))
    return out


def backward(g, f, x, W1, w2, act):
    """g: float; f: forward()'s dict -> dict: dz [T], da [T, D], dx [T, D], dW1 [D, D], db1 [D], dw2 [D], db2 []"""
    x, W1, w2 = _d(x), _d(W1), _d(w2).view(-1)
    gs = float(g) / f["n"] if f["n"] > 0 else 0.0
    dz = f["on"] * gs * (torch.sigmoid(f["z"]) - f["y"])
    da = dz[:, None] * w2[None, :] * act_grad_of(f["a"], act)
    return {"dz": dz, "da": da, "dx": da @ W1, "dW1": da.t() @ x, "db1": da.sum(0), "dw2": (dz[:, None] * f["h"]).sum(0),
            "db2": dz.sum()}


def bounds(g, f, r, x, W1, b1, w2, b2, act, K=None, prefill=None):
    """per-element bounds of an fp32 evaluation of everything forward() and backward() return (keys: a, h, z, row, loss, dz,
    da, dx, dW1, db1, dw2, db2).  f, r: forward()'s and backward()'s dicts (r None: forward only); prefill: {name: tensor} of
    what the parameter gradients held before (the sum is added to it)"""
    K = K_ULP if K is None else K
    x, W1, b1, w2, b2 = _d(x), _d(W1), _d(b1).view(-1), _d(w2).view(-1), _d(b2).view(-1)
    T, D = x.shape
    ax, aW, aw2 = x.abs(), W1.abs(), w2.abs()
    a, h, z = f["a"], f["h"], f["z"]
    B = {}
    B["a"] = (D + 2) * U * (b1.abs()[None, :] + ax @ aW.t())
    if act == RELU:
        B["h"] = B["a"].clone()
    else:
        B["h"] = 1.13 * B["a"] + (4 + K) * U * a.abs()
    B["z"] = B["h"] @ aw2 + (D + 2) * U * (b2.abs()[0] + h.abs() @ aw2)
    if "row" not in f:
        return B
    B["row"] = B["z"] + (4 + K) * U * (z.abs() + math.log(2.0))
    n, on = f["n"], f["on"]
    if n > 0:
        length = (T + 1023) // 1024 + 12         # the longest chain of the reduction: T / 1024 adds per thread, a tree of 10, the division
        B["loss"] = (B["row"] * on).sum() / n + length * U * (f["row"].abs() * on).sum() / n
    else:
        B["loss"] = torch.zeros((), dtype=F64)
    if r is None:
        return B
    gs = abs(float(g)) / n if n > 0 else 0.0
    sig_y = (torch.sigmoid(z) - f["y"]).abs()
    B["dz"] = on * gs * (0.25 * B["z"] + (6 + K) * U * sig_y)
    dz, da = r["dz"], r["da"]
    gp = act_grad_of(a, act).abs()
    if act == RELU:
        Bgp = (a.abs() <= B["a"]).to(F64)
    else:
        Bgp = 0.8 * B["a"] + (6 + K) * U * 1.25
    B["da"] = aw2[None, :] * (B["dz"][:, None] * gp + dz.abs()[:, None] * Bgp) + 3 * U * da.abs()
    B["dx"] = B["da"] @ aW + (D + 2) * U * (da.abs() @ aW)
    LT = T + 3
    B["dW1"] = B["da"].t() @ ax + LT * U * (da.abs().t() @ ax)
    B["db1"] = B["da"].sum(0) + LT * U * da.abs().sum(0)
    B["dw2"] = (B["dz"][:, None] * h.abs() + dz.abs()[:, None] * B["h"]).sum(0) + LT * U * (dz.abs()[:, None] * h.abs()).sum(0)
    B["db2"] = B["dz"].sum() + LT * U * dz.abs().sum()
    if prefill:
        for k, v in prefill.items():
            B[k] = B[k] + U * (_d(v).view(B[k].shape).abs() + r[k].abs())
    return B


def ratios(got, want, B):
    """{key: worst |got - want| / bound} over the keys of `got`; an element whose bound is 0 must be met exactly (ratio 0 if it
    is, inf if not)"""
    out = {}
    for k, v in got.items():
        e = (_d(v).view(want[k].shape) - want[k]).abs()
        b = B[k]
        q = torch.where(b > 0, e / b.clamp(min=1e-300), torch.where(e > 0, torch.full_like(e, float("inf")), torch.zeros_like(e)))
        out[k] = float(q.max()) if q.numel() else 0.0
    return out
