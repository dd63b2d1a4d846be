"""The Gumbel noise of the sampling heads (include/t4r_hip_sampling.h, csrc/gumbel_noise.h), restated in numpy over the oracle's
Philox4x32-10: block(key = seed, c0 = item, c1 = row >> 2, (c2, c3) = ctr_hi), word row & 3, u = ((w >> 9) + 0.5) 2^-23,
g = -log(-log u) in float64.  Shared by tests/test_sampling_cpu.py and tests/test_sampling_gpu.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
from device_rng import dropout_ctr_hi, philox4x32_10  # noqa: E402

SITE_GUMBEL = 7


def ctr_hi_of(offset):
    return dropout_ctr_hi(offset, 255, SITE_GUMBEL)


def uniforms(seed, ctr_hi, rows, items):
    """u [len(rows), len(items)] float64 (every value exact in fp32) for the stream rows `rows` and the item ids `items`"""
    rows = np.asarray(rows, dtype=np.uint64)
    items = np.asarray(items, dtype=np.uint64)
    ctr_lo = ((rows[:, None] >> np.uint64(2)) << np.uint64(32)) | items[None, :]
    w = philox4x32_10(seed, ctr_lo, ctr_hi)                                  # [R, C, 4]
    sel = np.broadcast_to((rows & np.uint64(3)).astype(np.int64)[:, None, None], (len(rows), len(items), 1))
    w = np.take_along_axis(w, sel, 2)[..., 0]
    return ((w >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel(seed, ctr_hi, rows, items):
    """g [len(rows), len(items)] float64"""
    return -np.log(-np.log(uniforms(seed, ctr_hi, rows, items)))


def chi2_of_argmax(picks, logits):
    """(Pearson chi^2 of the pick counts against softmax(logits), smallest expected count)"""
    logits = np.asarray(logits, dtype=np.float64)
    pr = np.exp(logits - logits.max())
    pr /= pr.sum()
    cnt = np.bincount(np.asarray(picks).reshape(-1), minlength=len(logits)).astype(np.float64)
    exp = cnt.sum() * pr
    return float(((cnt - exp) ** 2 / exp).sum()), float(exp.min())


CHI2_60_Q999 = 99.6          # the 0.999 quantile of chi^2 with 60 degrees of freedom (V = 61)


def freq_logits():
    """the V = 61 logits of the two frequency tests"""
    return np.random.default_rng(0).standard_normal(61) * 1.5


def fake_tokens_formula(itemid_seq, target_flat, drawn, padding_idx, sample_from_batch):
    """the integer part of the reference's get_fake_tokens (transformers4rec/torch/masking.py:816-848), restated with
    index assignment: (corrupted_inputs [B, L], discriminator_labels [B, L] bool, batch_updates)"""
    import torch

    L = itemid_seq.size(1)
    at = (target_flat != padding_idx).nonzero().flatten()
    pos_labels = target_flat[at]
    if sample_from_batch:
        batch_updates, updates = drawn, pos_labels[drawn]
    else:
        batch_updates, updates = [], drawn
    corrupted_labels = target_flat.clone()
    corrupted_labels[at] = updates
    corrupted_inputs = itemid_seq.clone().reshape(-1)
    corrupted_inputs[at] = updates
    return corrupted_inputs.view(-1, L), (corrupted_labels != target_flat).view(-1, L), batch_updates if torch.is_tensor(batch_updates) else []
