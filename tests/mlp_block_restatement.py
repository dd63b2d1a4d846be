"""float64 restatement of the MLP block (csrc/mlp_block.hip, include/t4r_hip_mlpblock.h), forward and gradients, the error bounds
its tests use, and planted faults that those bounds have to catch.  Host tensors only.

Symbols: x = a_{-1} [T, K_0]; layer i: W_i [N_i, K_i], b_i [N_i] or None, K_i = N_{i-1};
    z_i = b_i + a_{i-1} W_i^T,  r_i = max(z_i, 0) (relu) or z_i,  a_i = r_i keep_i s (p > 0) or r_i,  s = fl32(1 / (1 - fl32(p))),
    keep_i[t][d] = oracle.device_rng.dropout_keep(seed, dropout_ctr_hi(offset, layer = i, site = 8))[t N_i + d].

Bounds, EPS = 2^-24 (one fp32 rounding), derived from the arithmetic and valid for any order of the K_i terms:
    a_i    (K_i + 2) EPS (|b_i| + |a_{i-1}| |W_i|^T) s       a chain of K_i fused multiply-adds (each partial sum is at most the
                                                             sum of the magnitudes) and the one rounding of the scale; exact
                                                             zeros (dropped, or clipped by the ReLU away from z = 0) have error 0
    dz_i   |da_i| gate_i rounds once: EPS |dz_i|, plus the bound carried by da_i times gate_i
    da_{i-1} = dz_i W_i   (N_i + 2) EPS |dz_i| |W_i|  plus the bound carried by dz_i times |W_i|  (da_{n-1} = dout: exact)
    d W_i  (T + 3) EPS |dz_i|^T |a_{i-1}|  plus  (bound of dz_i)^T |a_{i-1}|  plus EPS |d W_i| for the add into the start value
    d b_i  (T + 3) EPS sum_t |dz_i|        plus  sum_t bound of dz_i          plus EPS |d b_i|
The forward is checked layer by layer on the DEVICE's own a_{i-1} (forward(..., acts=...)), so its bounds do not compound; the
backward's bounds are carried down the chain as written above, from the device's own activations."""
import numpy as np
import torch

import device_rng

EPS = 2.0 ** -24
SITE = 8
FAULTS = ("no_bias", "no_scale", "mask_transposed", "mask_prev_layer", "gate_from_z", "db_overwritten", "last_act_skipped")


def inv_keep(p):
    """the factor of a kept element as the device forms it: fl32(1 / (1 - fl32(p))); 1 for p = 0"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def keep_masks(seed, offset, T, dims, p, fault=None):
    """bool [T, N_i] per layer: the device's keep decisions (all True for p = 0)"""
    out = []
    for i, N in enumerate(dims):
        if p <= 0:
            out.append(torch.ones((T, N), dtype=torch.bool))
            continue
        layer = i - 1 if fault == "mask_prev_layer" else i
        k = torch.from_numpy(device_rng.dropout_keep(seed, device_rng.dropout_ctr_hi(offset, layer, SITE), T * N, p).astype(np.bool_))
        out.append(k.view(N, T).t().contiguous() if fault == "mask_transposed" else k.view(T, N))
    return out


def layer(a_prev, W, b, relu, keep, p, fault=None, last=False):
    """-> (a_i float64, bound) of one layer on the input a_prev"""
    a_prev, W = a_prev.double(), W.double()
    K = W.shape[1]
    s = inv_keep(p)
    z = a_prev @ W.t()
    A = a_prev.abs() @ W.abs().t()
    if b is not None:
        A = A + b.double().abs()
        if fault != "no_bias":
            z = z + b.double()
    r = z.clamp_min(0.0) if relu and not (fault == "last_act_skipped" and last) else z
    a = r * keep.double() * (1.0 if fault == "no_scale" else s)
    return a, (K + 2) * EPS * A * s


def forward(x, Ws, bs, relu, p, keeps, fault=None, acts=None):
    """-> list of (a_i float64, bound_i).  acts: the device's own stored activations; layer i then starts from acts[i - 1] and the
    bounds do not compound.  Without them each layer starts from the restated a_{i-1} (bounds then hold for layer 0 only)."""
    out, prev = [], x
    n = len(Ws)
    for i in range(n):
        a, bound = layer(prev, Ws[i], None if bs is None else bs[i], relu, keeps[i], p, fault, last=i == n - 1)
        out.append((a, bound))
        prev = a if acts is None else acts[i]
    return out


def backward(dout, x, Ws, bs, acts, relu, p, keeps, dW0=None, db0=None, fault=None):
    """-> dict dx: (value, bound), dW: [(value, bound)], db: [(value, bound)] from the activations `acts` (the device's own, or
    the restated ones); gradients are ADDED to the start values dW0[i], db0[i] where given"""
    n = len(Ws)
    T = dout.shape[0]
    s = inv_keep(p)
    da, bda = dout.double(), torch.zeros_like(dout, dtype=torch.float64)
    dW, db = [None] * n, [None] * n
    for i in reversed(range(n)):
        W = Ws[i].double()
        prev = (x if i == 0 else acts[i - 1]).double()
        if relu:
            if fault == "gate_from_z":
                z = prev @ W.t() + (0.0 if bs is None or bs[i] is None else bs[i].double())
                gate = (z > 0).double() * s
            else:
                gate = (acts[i].double() > 0).double() * s
        else:
            gate = keeps[i].double() * s
        dz = da * gate
        bdz = bda * gate + EPS * dz.abs()
        gw = dz.t() @ prev
        bw = (T + 3) * EPS * (dz.abs().t() @ prev.abs()) + bdz.t() @ prev.abs()
        gb = dz.sum(0)
        bb = (T + 3) * EPS * dz.abs().sum(0) + bdz.sum(0)
        if dW0 is not None:
            gw = gw + dW0[i].double()
            bw = bw + EPS * gw.abs()
        if db0 is not None and fault != "db_overwritten":
            gb = gb + db0[i].double()
            bb = bb + EPS * gb.abs()
        dW[i], db[i] = (gw, bw), (gb, bb)
        N = W.shape[0]
        da, bda = dz @ W, (N + 2) * EPS * (dz.abs() @ W.abs()) + bdz @ W.abs()
    return {"dx": (da, bda), "dW": dW, "db": db}


def ratio(got, want, bound):
    """worst error / bound of an fp32 result against its float64 restatement (0 where both error and bound are 0)"""
    err = (got.double() - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


def make_case(T, K0, dims, bias=True, seed=0):
    """inputs of one case: x, dout, W_i and b_i as torch.nn.Linear draws them, and non-zero start values of the gradients"""
    g = torch.Generator().manual_seed(seed * 7919 + T * 1000003 + K0 * 10007 + sum((j + 1) * d for j, d in enumerate(dims)))
    Ws, bs, dW0, db0 = [], [], [], []
    k = K0
    for N in dims:
        lim = 1.0 / k ** 0.5
        Ws.append((torch.rand((N, k), generator=g) * 2 - 1) * lim)
        bs.append((torch.rand((N,), generator=g) * 2 - 1) * lim if bias else None)
        dW0.append(torch.randn((N, k), generator=g))
        db0.append(torch.randn((N,), generator=g))
        k = N
    return dict(x=torch.randn((T, K0), generator=g), dout=torch.randn((T, dims[-1]), generator=g), Ws=Ws, bs=bs, dW0=dW0, db0=db0)


def torch_chain(k, relu, p, keeps):
    """the reference's chain in fp32 torch on the host (F.linear, relu, the given keep mask times fl32(1 / (1 - p)), autograd) ->
    (acts, grads dict with the start values added)"""
    x = k["x"].clone().requires_grad_()
    Ws = [w.clone().requires_grad_() for w in k["Ws"]]
    bs = [None if b is None else b.clone().requires_grad_() for b in k["bs"]]
    s = torch.tensor(inv_keep(p), dtype=torch.float32)
    acts, a = [], x
    for i, W in enumerate(Ws):
        a = torch.nn.functional.linear(a, W, bs[i])
        if relu:
            a = torch.relu(a)
        if p > 0:
            a = a * (keeps[i].float() * s)
        acts.append(a)
    a.backward(k["dout"])
    return ([t.detach() for t in acts],
            dict(dx=x.grad, dW=[w.grad + g0 for w, g0 in zip(Ws, k["dW0"])],
                 db=[None if b is None else b.grad + g0 for b, g0 in zip(bs, k["db0"])]))
