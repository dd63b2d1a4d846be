"""A lazy (row-sparse) Adam in numpy float64: the arithmetic csrc/row_adam.hip is held to, written from torch.optim.Adam's
formula and torch.optim.SparseAdam's "touched rows only" rule, independently of the kernel.

    g_r   = grad_scale * sum of rows[i] over ids[i] == r, in lookup order        (ids equal to padding_idx or outside [0, V) skipped)
    coupled weight decay:    g_r += weight_decay * p_r
    decoupled weight decay:  p_r *= 1 - lr * weight_decay
    m_r = b1 m_r + (1 - b1) g_r ;  v_r = b2 v_r + (1 - b2) g_r^2
    p_r -= lr / (1 - b1^t) * m_r / (sqrt(v_r) / sqrt(1 - b2^t) + eps)              t = the GLOBAL step, 1-based

for the rows r that some id names; every other row of p, m and v is left alone.

The reference is this at float64.  The same statements at float32 (p, m, v and rows given as float32 arrays: numpy keeps every
intermediate in float32) are the plain-fp32 yardstick of the error bound, the part torch's fp32 CPU Adam plays in
tests/test_adam_gpu.py -- torch has no lazy Adam with this formula (torch.optim.SparseAdam adds eps to sqrt(v) before the bias
correction, not after).
"""
import numpy as np


def summed_rows(V, ids, rows, padding_idx=-1, dtype=np.float64):
    """-> (sorted distinct valid ids, [U, D] sums in lookup order, in `dtype`)"""
    ids = np.asarray(ids).reshape(-1)
    rows = np.asarray(rows, dtype=dtype)
    sums = {}
    for i, r in enumerate(ids.tolist()):
        if r == padding_idx or r < 0 or r >= V:
            continue
        if r in sums:
            sums[r] = sums[r] + rows[i]
        else:
            sums[r] = rows[i].copy()
    touched = sorted(sums)
    D = rows.shape[1] if rows.ndim == 2 else 0
    return np.asarray(touched, dtype=np.int64), (np.stack([sums[r] for r in touched]) if touched else np.zeros((0, D), dtype=dtype))


def lazy_adam_step(p, m, v, ids, rows, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False,
                   grad_scale=1.0, padding_idx=-1):
    """in place on the arrays p, m, v [V, D], all float64 (the reference) or all float32 (the yardstick); -> the touched row ids"""
    assert p.dtype in (np.float64, np.float32) and m.dtype == p.dtype and v.dtype == p.dtype and step >= 1
    b1, b2 = betas
    touched, g = summed_rows(p.shape[0], ids, rows, padding_idx, p.dtype)
    if touched.size == 0:
        return touched
    g = g * grad_scale
    pr, mr, vr = p[touched], m[touched], v[touched]
    if decoupled:
        pr = pr * (1.0 - lr * weight_decay)
    else:
        g = g + weight_decay * pr
    mr = b1 * mr + (1.0 - b1) * g
    vr = b2 * vr + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    pr = pr - (lr / bc1) * mr / (np.sqrt(vr) / np.sqrt(bc2) + eps)
    p[touched], m[touched], v[touched] = pr, mr, vr
    return touched
