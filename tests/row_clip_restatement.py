"""Global-norm clipping over dense buckets and lazily stepped tables in numpy: the arithmetic csrc/row_adam.hip's two halves
(t4r_row_adam_reduce / t4r_row_adam_apply) and optim.FusedAdam(max_grad_norm=).link(RowSparseAdam) are held to, written from
torch.nn.utils.clip_grad_norm_'s formula and tests/row_adam_restatement.py's lazy Adam, independently of the kernels.

    g_r      = sum of rows[i] over ids[i] == r, in lookup order                 (a table's dense gradient: zero in every other row)
    norm     = |grad_scale| * sqrt(sum over the buckets of g^2 + sum over the tables and their named rows of g_r^2)
    coef     = min(max_norm / (norm + 1e-6), 1)
    every bucket and every named row then takes its Adam / AdamW step with the gradient (g * grad_scale) * coef

The reference is this at float64.  At float32 (arrays and coefficient given as float32: numpy keeps every intermediate in
float32, and the two products are two roundings as on the device) it is the plain-fp32 yardstick of the error bound.
"""
import numpy as np

import row_adam_restatement as ra


def sumsq64(x):
    """sum of squares in float64 of an array of any float type"""
    x = np.asarray(x, dtype=np.float64)
    return float((x * x).sum())


def joint_norm(buckets, tables, grad_scale=1.0):
    """float64 norm of the scaled gradient over `buckets` (arrays) and `tables` ([(V, ids, rows, padding_idx)]: the rows are
    summed per id in float64 first)"""
    s = sum(sumsq64(b) for b in buckets)
    for V, ids, rows, pad in tables:
        s += sumsq64(ra.summed_rows(V, ids, rows, pad, np.float64)[1])
    return abs(grad_scale) * np.sqrt(s)


def coef64(norm, max_norm):
    return min(max_norm / (norm + 1e-6), 1.0)


def coef32(norm, max_norm):
    """clip_grad_norm_'s fp32 arithmetic on the norm rounded to fp32 (tests/test_optim_clip_gpu.py: coef_of)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.minimum(np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6)), np.float32(1.0))


def clipped_lazy_adam_step(p, m, v, ids, rows, step, coef, grad_scale=1.0, padding_idx=-1, **hp):
    """ra.lazy_adam_step with the coefficient folded in: the per-row sums, times grad_scale, times coef -- in p's dtype, so
    two roundings at float32 -- go in as one lookup per named row.  In place; -> the touched row ids"""
    touched, g = ra.summed_rows(p.shape[0], ids, rows, padding_idx, p.dtype)
    if touched.size == 0:
        return touched
    g = (g * p.dtype.type(grad_scale)) * p.dtype.type(coef)
    return ra.lazy_adam_step(p, m, v, touched, g, step, grad_scale=1.0, padding_idx=-1, **hp)


def clipped_adam_step(p, m, v, grad, step, coef, grad_scale=1.0, **hp):
    """a dense bucket [n]: every element is a named row of width 1"""
    n = p.shape[0]
    clipped_lazy_adam_step(p.reshape(n, 1), m.reshape(n, 1), v.reshape(n, 1), np.arange(n), np.asarray(grad, dtype=p.dtype).reshape(n, 1),
                           step, coef, grad_scale, **hp)
