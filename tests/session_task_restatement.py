"""float64 restatement of the session-level task kernels (csrc/seq_task.hip, include/t4r_hip_seqtask.h) and the error bounds
their tests use.  Nothing here runs on the GPU; every function takes and returns CPU tensors (float64 inside).

Semantics (the header's): n_b = L without `lengths`, else min(max(len_b, 0), L);
    first  s_b = x[b, 0]          last  s_b = x[b, n_b - 1]          mean  s_b = sum_{l < n_b} x[b, l] / n_b          n_b = 0: s_b = 0
    z_b = bias + w . s_b          pred_b = sigmoid(z_b) (act 1) | z_b (act 0)
    MSE row (pred - t)^2          BCE row -(t max(log p, -100) + (1 - t) max(log(1 - p), -100))          loss = mean of the rows
    MSE dz = (g / B) 2 (pred - t) [times p (1 - p) under act 1]          BCE dz = (g / B) (p - t) p (1 - p) / max(p (1 - p), 1e-12)
    dx[b, l] = dz_b c_bl w        d_w = sum_b dz_b s_b        d_b = sum_b dz_b
"""
import torch

FIRST, LAST, MEAN = 0, 1, 2
MSE, BCE = 0, 1
U = 2.0 ** -24          # fp32 unit roundoff


def counts(B, L, lengths=None):
    if lengths is None:
        return torch.full((B,), L, dtype=torch.int64)
    return lengths.to(torch.int64).clamp(min=0, max=L)


def coef(B, L, summary, lengths=None):
    """c [B, L] float64: the weight of position l in session b's summary (and in its dx)"""
    n = counts(B, L, lengths)
    l = torch.arange(L)[None]
    c = torch.zeros(B, L, dtype=torch.float64)
    if summary == FIRST:
        c[:, 0] = 1.0
    elif summary == LAST:
        c[torch.arange(B), (n - 1).clamp(min=0)] = 1.0
    else:
        c = (l < n[:, None]).double() / n.clamp(min=1)[:, None].double()
    c[n == 0] = 0.0
    return c


def summary_of(x, summary, lengths=None):
    B, L, _D = x.shape
    return (coef(B, L, summary, lengths)[:, :, None] * x.double()).sum(1)


def logits(s, w, bias=None):
    z = s.double() @ w.double().reshape(-1)
    return z if bias is None else z + bias.double().reshape(())


def predictions(z, act):
    return torch.sigmoid(z.double()) if act else z.double()


def row_losses(pred, target, loss_kind):
    p, t = pred.double(), target.double()
    if loss_kind == MSE:
        return (p - t) ** 2
    return -(t * torch.log(p).clamp(min=-100.0) + (1.0 - t) * torch.log1p(-p).clamp(min=-100.0))


def dz_of(pred, target, g, act, loss_kind):
    p, t = pred.double(), target.double()
    gs = float(g) / p.shape[0]
    pq = p * (1.0 - p)
    d = gs * 2.0 * (p - t) if loss_kind == MSE else gs * (p - t) / pq.clamp(min=1e-12)
    return d * pq if act else d


def forward(x, w, bias, target, summary, act, loss_kind, lengths=None):
    """-> dict(s, z, pred, rows, loss), all float64"""
    s = summary_of(x, summary, lengths)
    z = logits(s, w, bias)
    pred = predictions(z, act)
    out = dict(s=s, z=z, pred=pred)
    if target is not None:
        out["rows"] = row_losses(pred, target, loss_kind)
        out["loss"] = out["rows"].mean()
    return out


def backward(dz, s, w, L, summary, lengths=None):
    """-> (dx [B, L, D], d_w [D], d_b []) float64 from given dz [B] and s [B, D]"""
    B = dz.shape[0]
    c = coef(B, L, summary, lengths)
    dx = (dz.double()[:, None] * c)[:, :, None] * w.double().reshape(1, 1, -1)
    return dx, (dz.double()[:, None] * s.double()).sum(0), dz.double().sum()


# ------------------------------------------------------------------------------------------------ bounds
def z_bound(x, w, summary, lengths=None):
    """per row: (L + D + 8) u sum_d |w_d| mean_l |x_ld| -- the mean over the positions the summary reads (L of them at most, one
    fp32 chain), then a D-term dot product and the bias"""
    B, L, D = x.shape
    mag = (coef(B, L, summary, lengths)[:, :, None] * x.double().abs()).sum(1) @ w.double().abs().reshape(-1)
    return (L + D + 8) * U * mag


def pred_bound(zb, pred, act):
    """z's bound through the activation (|sigmoid'| <= 1/4; identity: 1) plus 8 u |value| for the device's exp and the divide"""
    return (0.25 * zb if act else zb) + 8 * U * pred.double().abs()
