"""float64 restatement of the continuous-feature projection's first layer (csrc/cont_proj.hip) and the error bounds its tests
use.  Host tensors only."""
import torch

EPS = 2.0 ** -24        # half an ulp of fp32: the relative error of one rounding


def stack(xs, per_session, L):
    """the [T, C] operand the kernel never writes: column c is xs[c] flattened, a per-session column repeated over L"""
    cols = []
    for x, flag in zip(xs, per_session):
        x = x.double().reshape(-1)
        cols.append(x.repeat_interleave(L) if flag else x)
    return torch.stack(cols, dim=1)


def forward(xs, per_session, L, W, b):
    """-> (y [T, P] float64, bound [T, P]): relu(b + X W^T) and the FMA-chain bound (C + 2) eps (|b| + |X| |W|^T) on the fp32
    result (a chain of C fused multiply-adds from b has at most C roundings; ReLU is 1-Lipschitz)"""
    X = stack(xs, per_session, L)
    W, b = W.double(), b.double()
    y = torch.relu(b + X @ W.t())
    bound = (X.shape[1] + 2) * EPS * (b.abs() + X.abs() @ W.abs().t())
    return y, bound


def gradients(xs, per_session, L, g, mask):
    """d W, d b of the layer for the output gradient g [T, P] under the given ReLU mask [T, P] (bool), with the bounds
    (T + 2) eps sum_t |g x| and (T + 2) eps sum_t |g|, valid for any summation order of fp32 products and sums"""
    X = stack(xs, per_session, L)
    gm = g.double() * mask.double()
    T = X.shape[0]
    dW, db = gm.t() @ X, gm.sum(0)
    return dW, db, (T + 2) * EPS * (gm.abs().t() @ X.abs()), (T + 2) * EPS * gm.abs().sum(0)
