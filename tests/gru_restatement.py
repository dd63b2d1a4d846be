"""float64 restatement of the GRU body (csrc/gru.hip, include/t4r_hip_gru.h), forward and gradients, the error bounds its tests
use, and planted faults that those bounds have to catch.  Host tensors only.

Symbols: x = a^0 [B, L, K_0]; layer k: W_ih [3H, K_k], W_hh [3H, H], b_ih, b_hh [3H] or None (gate order r | z | n), K_k = H above;
    gi_t = b_ih + W_ih a_t,  gh_t = b_hh + W_hh h_{t-1},  h_{-1} = h0[k] (None: zeros)
    r = sig(gi_r + gh_r),  z = sig(gi_z + gh_z),  n = tanh(gi_n + r gh_n),  h_t = n + z (h_{t-1} - n)
    a^{k+1} = h^k keep_k s (p > 0, k < n - 1) or h^k,  s = fl32(1 / (1 - fl32(p))),
    keep_k[(b L + t) H + d] = oracle.device_rng.dropout_keep(seed, dropout_ctr_hi(offset, layer = k, site = 9)).

Bounds, EPS = 2^-24 (one fp32 rounding).  A product of K terms seeded with the bias is bounded by (K + 2) EPS (|b| + |a| |W|^T),
valid for any order of the terms.  The bound of a pre-activation passes through sig with the factor 1/4 and through tanh with
the factor 1 (their largest slopes: exact by the mean value theorem, not first order).  Each evaluation of sig / tanh adds an
absolute allowance U EPS, derived for the expressions the kernel uses (include/t4r_hip_gru.h) from the accuracy limits of the
device functions they call -- expf 3 ulp, / 2.5 ulp (the OpenCL limits, which ROCm's device library meets), + and - half an
ulp; one ulp is at most 2 EPS relative:
    sig(v) = 1 / (1 + expf(-v)):   e = expf(-v) is off by 6 EPS e;  s = 1 + e by 6 EPS e + EPS s <= 7 EPS s;  1 / s by 7 EPS +
        5 EPS relative; sig <= 1, so U_SIG = 12.
    tanh(v) = 1 - 2 / (1 + expf(2 v)):   q = 2 / (1 + e) is off by 12 EPS q as above, q <= 2: 24 EPS; the subtraction rounds once,
        |tanh| <= 1: U_TANH = 25.   (An overflowing expf gives q = 0 and tanh = 1, off by less than 2^-126.)
    h = n + z (hp - n), hp exact:   (1 - z) B_n + |hp - n| B_z + EPS (z |hp - n| + |z (hp - n)| + |h|)
The forward is checked step by step from the DEVICE's own h_{t-1} (forward(..., h_dev=...)), so its bounds do not compound over
L.  The backward's bounds are carried along the dh chain, from the device's own h and the float64 gate values; the forward
bounds B_r, B_z, B_n, B_ghn stand for what the device's stored gate values may differ by:
    dh = dy + carry                      b_dy + b_carry + EPS |dh|
    dpre_n = dh (1 - z)(1 - n n)         b_dh (1-z)(1-nn) + |dh| (B_z + EPS (1-z)) (1-nn) + |dh| (1-z)(2 |n| B_n + EPS) + 2 EPS |.|
    dpre_z = dh (hp - n) z (1 - z)       b_dh |c| D + |dh| (B_n + EPS |c|) D + |dh| |c| (|1 - 2z| B_z + 2 EPS D) + 2 EPS |.|
    dpre_r = dpre_n gh_n r (1 - r)       b_n |gh| E + |dpre_n| B_ghn E + |dpre_n| |gh| (|1 - 2r| B_r + 2 EPS E) + 2 EPS |.|
    dgh_n  = dpre_n r                    b_n r + |dpre_n| B_r + EPS |.|
    carry' = dh z + W_hh^T dgh           b_dh z + |dh| B_z + EPS |dh z| + (3H + 2) EPS (|dh z| + |W_hh|^T |dgh|) + |W_hh|^T b_dgh
    d a    = dgi W_ih                    (3H + 2) EPS |dgi| |W_ih| + b_dgi |W_ih|
    d W    = sum dg^T [a | 1]            (T + 3) EPS |dg|^T |a| + b_dg^T |a| + EPS |d W| for the add into the start value
Products of two bounds are of second order; every bound is multiplied by SECOND = 1.01 for them.  The carried bound grows per
step by about max(z + |W_hh|^T |slopes|); make_case draws W_hh at a scale that keeps it near 1 (see there)."""
import numpy as np
import torch

import device_rng

EPS = 2.0 ** -24
SITE = 9
U_SIG, U_TANH = 12.0, 25.0
SECOND = 1.01
FWD_FAULTS = ("gates_zr", "bhn_outside", "blend_swapped", "drop_state", "mask_prev_layer", "mask_transposed", "h0_ignored")
BWD_FAULTS = ("bptt_truncated", "dbhh_n_from_dbih", "grad_overwritten")
FAULTS = FWD_FAULTS + BWD_FAULTS


def inv_keep(p):
    """the factor of a kept element as the device forms it: fl32(1 / (1 - fl32(p))); 1 for p = 0"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def keep_masks(seed, offset, B, L, H, n, p, fault=None):
    """bool [B, L, H] per layer below the last: the device's keep decisions (all True for p = 0)"""
    out = []
    for k in range(n - 1):
        if p <= 0:
            out.append(torch.ones((B, L, H), dtype=torch.bool))
            continue
        layer = k + 1 if fault == "mask_prev_layer" else k
        m = torch.from_numpy(device_rng.dropout_keep(seed, device_rng.dropout_ctr_hi(offset, layer, SITE), B * L * H, p).astype(np.bool_))
        out.append(m.view(H, B * L).t().contiguous().view(B, L, H) if fault == "mask_transposed" else m.view(B, L, H))
    return out


def dropped(h32, keep, p):
    """the next layer's input exactly as the device forms it from its own h: one fp32 multiply by 0 or fl32(1 / (1 - p))"""
    if p <= 0:
        return h32
    if h32.dtype != torch.float32:                        # restated values: carried in float64
        return h32 * keep.double() * inv_keep(p)
    return h32 * (keep.float() * torch.tensor(inv_keep(p), dtype=torch.float32))


def _lin(a, W, b, K):
    """b + a W^T in float64 and its (K + 2) EPS bound"""
    v = a @ W.t()
    A = a.abs() @ W.abs().t()
    if b is not None:
        v, A = v + b, A + b.abs()
    return v, (K + 2) * EPS * A


def step(a_t, hp, W_ih, W_hh, b_ih, b_hh, fault=None):
    """one step of one layer on the input a_t [B, K] and the state hp [B, H] (float64) -> dict of float64 values and bounds"""
    H, K = W_hh.shape[1], W_ih.shape[1]
    gi, Bgi = _lin(a_t, W_ih, b_ih, K)
    if fault == "bhn_outside" and b_hh is not None:
        gh, Bgh = _lin(hp, W_hh, torch.cat([b_hh[:2 * H], torch.zeros_like(b_hh[2 * H:])]), H)
        gi = gi + torch.cat([torch.zeros_like(b_hh[:2 * H]), b_hh[2 * H:]])
    else:
        gh, Bgh = _lin(hp, W_hh, b_hh, H)
    o = (1, 0, 2) if fault == "gates_zr" else (0, 1, 2)
    sl = [slice(j * H, (j + 1) * H) for j in o]
    pr, pz = gi[:, sl[0]] + gh[:, sl[0]], gi[:, sl[1]] + gh[:, sl[1]]
    r, z = torch.sigmoid(pr), torch.sigmoid(pz)
    Br = (Bgi[:, sl[0]] + Bgh[:, sl[0]] + EPS * pr.abs()) / 4 + U_SIG * EPS
    Bz = (Bgi[:, sl[1]] + Bgh[:, sl[1]] + EPS * pz.abs()) / 4 + U_SIG * EPS
    ghn, Bghn = gh[:, sl[2]], Bgh[:, sl[2]]
    pn = gi[:, sl[2]] + r * ghn
    n = torch.tanh(pn)
    Bn = Bgi[:, sl[2]] + ghn.abs() * Br + r * Bghn + EPS * (r * ghn).abs() + EPS * pn.abs() + U_TANH * EPS
    c = hp - n
    h = hp + z * (n - hp) if fault == "blend_swapped" else n + z * c
    Bh = (1 - z) * Bn + c.abs() * Bz + EPS * (z * c.abs() + (z * c).abs() + h.abs())
    return dict(r=r, z=z, n=n, ghn=ghn, h=h, pr=pr, pz=pz, pn=pn, Br=Br * SECOND, Bz=Bz * SECOND, Bn=Bn * SECOND, Bghn=Bghn * SECOND,
                Bh=Bh * SECOND)


def _p64(ts):
    return None if ts is None else [None if t is None else t.double() for t in ts]


def forward(x, W_ih, W_hh, b_ih, b_hh, h0, p, keeps, fault=None, h_dev=None):
    """-> per layer a dict: h [B, L, H] float64, Bh its bound, and the gate values r, z, n, ghn with their bounds.
    h_dev: the device's own h of every layer (fp32, [B, L, H] each); step t of layer k then starts from h_dev[k][:, t - 1] and the
    layer's input is formed from h_dev[k - 1]: the bounds do not compound.  Without it the restated values are carried."""
    n_layers = len(W_ih)
    W_ih, W_hh, b_ih, b_hh = _p64(W_ih), _p64(W_hh), _p64(b_ih), _p64(b_hh)
    B, L = x.shape[0], x.shape[1]
    H = W_hh[0].shape[1]
    a, out = x.double(), []
    for k in range(n_layers):
        bi, bh = (None if b_ih is None else b_ih[k]), (None if b_hh is None else b_hh[k])
        hp = torch.zeros((B, H), dtype=torch.float64) if h0 is None or fault == "h0_ignored" else h0[k].double()
        keys = ("r", "z", "n", "ghn", "h", "Br", "Bz", "Bn", "Bghn", "Bh", "pr", "pz", "pn")
        acc = {key: [] for key in keys}
        for t in range(L):
            s = step(a[:, t], hp, W_ih[k], W_hh[k], bi, bh, fault)
            for key in keys:
                acc[key].append(s[key])
            hp = s["h"] if h_dev is None else h_dev[k][:, t].double()
            if fault == "drop_state" and k < n_layers - 1 and p > 0:
                hp = hp * keeps[k][:, t].double() * inv_keep(p)
        lay = {key: torch.stack(v, 1) for key, v in acc.items()}
        out.append(lay)
        if k < n_layers - 1:
            a = (dropped(h_dev[k], keeps[k], p).double() if h_dev is not None else lay["h"] * keeps[k].double() * inv_keep(p))
    return out


def backward(dout, x, W_ih, W_hh, h0, hs, fwd, p, keeps, g0=None, fault=None):
    """-> dict dx: (value, bound), and W_ih, W_hh, b_ih, b_hh: lists of (value, bound) per layer.  hs: every layer's h [B, L, H] (the
    device's own, or the restated ones); fwd: forward(...)'s result on them (gate values and their bounds); g0: start values
    {name: [tensor per layer]} the gradients are ADDED to."""
    n_layers = len(W_ih)
    W_ih, W_hh = _p64(W_ih), _p64(W_hh)
    B, L, H = hs[0].shape
    T = B * L
    res = {key: [None] * n_layers for key in ("W_ih", "W_hh", "b_ih", "b_hh")}
    dy, bdy = dout.double(), torch.zeros(dout.shape, dtype=torch.float64)
    for k in reversed(range(n_layers)):
        f, Whh = fwd[k], W_hh[k]
        h = hs[k].double()
        a = (x if k == 0 else dropped(hs[k - 1], keeps[k - 1], p)).double()
        h_first = torch.zeros((B, 1, H), dtype=torch.float64) if h0 is None else h0[k].double().unsqueeze(1)
        hprev = torch.cat([h_first, h[:, :-1]], 1)
        carry, bcarry = torch.zeros((B, H), dtype=torch.float64), torch.zeros((B, H), dtype=torch.float64)
        dgi, bgi, dgh, bgh = [None] * L, [None] * L, [None] * L, [None] * L
        for t in reversed(range(L)):
            r, z, n, gh, hp = f["r"][:, t], f["z"][:, t], f["n"][:, t], f["ghn"][:, t], hprev[:, t]
            Br, Bz, Bn, Bg = f["Br"][:, t], f["Bz"][:, t], f["Bn"][:, t], f["Bghn"][:, t]
            dh = dy[:, t] + carry
            bdh = bdy[:, t] + bcarry + EPS * dh.abs()
            A, Bv, c, D, E = 1 - z, 1 - n * n, hp - n, z * (1 - z), r * (1 - r)
            dpn = dh * A * Bv
            bn = bdh * A * Bv + dh.abs() * (Bz + EPS * A) * Bv + dh.abs() * A * (2 * n.abs() * Bn + EPS) + 2 * EPS * dpn.abs()
            dpz = dh * c * D
            bz = bdh * c.abs() * D + dh.abs() * (Bn + EPS * c.abs()) * D + dh.abs() * c.abs() * ((1 - 2 * z).abs() * Bz + 2 * EPS * D) \
                + 2 * EPS * dpz.abs()
            dpr = dpn * gh * E
            br = bn * gh.abs() * E + dpn.abs() * Bg * E + dpn.abs() * gh.abs() * ((1 - 2 * r).abs() * Br + 2 * EPS * E) + 2 * EPS * dpr.abs()
            dgn = dpn * r
            bgn = bn * r + dpn.abs() * Br + EPS * dgn.abs()
            dgi[t], bgi[t] = torch.cat([dpr, dpz, dpn], 1), torch.cat([br, bz, bn], 1) * SECOND
            dgh[t], bgh[t] = torch.cat([dpr, dpz, dgn], 1), torch.cat([br, bz, bgn], 1) * SECOND
            acc0 = dh * z
            carry = acc0 + dgh[t] @ Whh
            bcarry = (bdh * z + dh.abs() * Bz + EPS * acc0.abs() + (3 * H + 2) * EPS * (acc0.abs() + dgh[t].abs() @ Whh.abs())
                      + bgh[t] @ Whh.abs()) * SECOND
            if fault == "bptt_truncated":
                carry = torch.zeros_like(carry)
        dgi, bgi, dgh, bgh = (torch.stack(v, 1).reshape(T, 3 * H) for v in (dgi, bgi, dgh, bgh))
        a2, hp2 = a.reshape(T, -1), hprev.reshape(T, H)

        def wsum(g, bg, src, name):
            gw = g.t() @ src
            bw = (T + 3) * EPS * (g.abs().t() @ src.abs()) + bg.t() @ src.abs()
            if g0 is not None and g0.get(name) is not None and g0[name][k] is not None and fault != "grad_overwritten":
                gw = gw + g0[name][k].double().reshape(gw.shape)
                bw = bw + EPS * gw.abs()
            return gw, bw * SECOND
        ones = torch.ones((T, 1), dtype=torch.float64)
        res["W_ih"][k] = wsum(dgi, bgi, a2, "W_ih")
        res["W_hh"][k] = wsum(dgh, bgh, hp2, "W_hh")
        gb, bb = wsum(dgi, bgi, ones, "b_ih")
        res["b_ih"][k] = (gb.reshape(-1), bb.reshape(-1))
        src_g, src_b = (dgh, bgh)
        if fault == "dbhh_n_from_dbih":
            src_g = torch.cat([dgh[:, :2 * H], dgi[:, 2 * H:]], 1)
        gb, bb = wsum(src_g, src_b, ones, "b_hh")
        res["b_hh"][k] = (gb.reshape(-1), bb.reshape(-1))
        Wih = W_ih[k]
        da = (dgi @ Wih).reshape(B, L, -1)
        bda = (((3 * H + 2) * EPS * (dgi.abs() @ Wih.abs()) + bgi @ Wih.abs()) * SECOND).reshape(B, L, -1)
        if k > 0:
            m = keeps[k - 1].double() * inv_keep(p)
            dy, bdy = da * m, bda * m + (EPS * (da * m).abs() if p > 0 else 0.0)
        else:
            res["dx"] = (da, bda)
    return res


def ratio(got, want, bound):
    """worst error / bound of an fp32 result against its float64 restatement (0 where both error and bound are 0)"""
    err = (got.double() - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


def make_case(B, L, K0, H, n, bias=True, with_h0=False, seed=0, x_scale=1.0, whh_scale=None):
    """inputs of one case.  W_ih and the biases as torch.nn.GRU draws them, U(-1/sqrt(H), 1/sqrt(H)).  W_hh is drawn U(-w, w) with
    w = min(1/sqrt(H), 2/H) unless whh_scale gives w: the backward's carried bound grows per step by about
    z + |W_hh|^T |slopes| ~ 0.5 + 0.4 (w H / 2); with torch's scale that is 0.5 + 0.2 sqrt(H) > 1 (a bound that doubles every step says
    nothing after 20), with w <= 2/H it is about 0.9.  The arithmetic tested is the same; the fixtures replay torch's own scale."""
    g = torch.Generator().manual_seed(seed * 7919 + B * 1000003 + L * 10007 + K0 * 101 + H * 7 + n)
    lim = 1.0 / H ** 0.5
    w = min(lim, 2.0 / H) if whh_scale is None else whh_scale
    u = lambda shape, s: (torch.rand(shape, generator=g) * 2 - 1) * s  # noqa: E731
    W_ih = [u((3 * H, K0 if k == 0 else H), lim) for k in range(n)]
    W_hh = [u((3 * H, H), w) for k in range(n)]
    b_ih = [u((3 * H,), lim) for k in range(n)] if bias else None
    b_hh = [u((3 * H,), lim) for k in range(n)] if bias else None
    g0 = {"W_ih": [torch.randn(t.shape, generator=g) for t in W_ih], "W_hh": [torch.randn(t.shape, generator=g) for t in W_hh],
          "b_ih": [torch.randn((3 * H,), generator=g) for _ in range(n)] if bias else None,
          "b_hh": [torch.randn((3 * H,), generator=g) for _ in range(n)] if bias else None}
    return dict(x=torch.randn((B, L, K0), generator=g) * x_scale, dout=torch.randn((B, L, H), generator=g), W_ih=W_ih, W_hh=W_hh,
                b_ih=b_ih, b_hh=b_hh, h0=u((n, B, H), 1.0) if with_h0 else None, g0=g0)


def fp32_standin(k, p, keeps):
    """a stand-in for the device on the host: the restatement carried in float64 and rounded to fp32 per layer -> list of h"""
    f = forward(k["x"], k["W_ih"], k["W_hh"], k["b_ih"], k["b_hh"], k["h0"], p, keeps)
    return [lay["h"].float() for lay in f]
