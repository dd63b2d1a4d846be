"""The pretrained-embedding projection (include/t4r_hip_pretrained.h) and its gradients restated with torch on the CPU, from the
image's exact values (`image.float()`): in float64 the yardstick, in float32 (`F.linear` + `F.layer_norm`, torch autograd) the
figure the kernels' error is compared with."""
import torch
import torch.nn.functional as F


def token_ids(ids, T):
    """ids [T / ids_div] -> the id of each of the T tokens"""
    ids = ids.reshape(-1)
    return ids.repeat_interleave(T // ids.numel())


def forward(image, ids, T, W, b, gamma=None, beta=None, eps=1e-5, dtype=torch.float64):
    """-> out [T, P] in `dtype`; image [V, E] fp16 (CPU), ids int64"""
    x = image.float().to(dtype)[token_ids(ids, T)]
    z = F.linear(x, W.to(dtype), b.to(dtype))
    if gamma is not None:
        z = F.layer_norm(z, (W.shape[0],), gamma.to(dtype), beta.to(dtype), eps)
    return z


def gradients(image, ids, T, W, b, gamma, beta, dY, eps=1e-5, dtype=torch.float64):
    """-> dict(dW, db[, dgamma, dbeta]) of sum(out * dY) in `dtype` by torch autograd"""
    ps = dict(dW=W.to(dtype).clone().requires_grad_(True), db=b.to(dtype).clone().requires_grad_(True))
    if gamma is not None:
        ps["dgamma"] = gamma.to(dtype).clone().requires_grad_(True)
        ps["dbeta"] = beta.to(dtype).clone().requires_grad_(True)
    x = image.float().to(dtype)[token_ids(ids, T)]
    z = F.linear(x, ps["dW"], ps["db"])
    if gamma is not None:
        z = F.layer_norm(z, (W.shape[0],), ps["dgamma"], ps["dbeta"], eps)
    (z * dY.to(dtype)).sum().backward()
    return {k: p.grad for k, p in ps.items()}


def rel_err(x, ref64):
    """largest error divided by the largest |reference|"""
    den = float(ref64.abs().max())
    return float((x.double() - ref64).abs().max()) / (den if den > 0 else 1.0)
