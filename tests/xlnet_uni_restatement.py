"""XLNet with attn_type='uni' restated in torch on the CPU: the causal relative-attention core (float64 reference and
per-element bounds), the layer and the model with a causal flag, and the training-mode form fed with the device's keep masks.
No GPU, no HIP library.

The reduction (HF modeling_xlnet.py create_mask :895-925, relative_positional_encoding :940-976, rel_shift_bnij :81-93): 'uni'
masks key j of row i when j > i and keeps the relative positions L .. 0, the first L + 1 rows of the 'bi' encoding; a live pair
(j <= i) reads row j - i + L in [1, L] -- the index the bi restatement uses.  So every formula here is the bi one with the dead
set extended by j > i (tests/test_xlnet_uni_cpu.py holds the model against the installed HF XLNetModel(attn_type='uni')).

Core: `reference` and `bounds` are those of tests/attn_core_restatement.py (formulas, MULT = 0.5 and C_EXP = 0 in its
docstring), called with its `xlnet_dead` replaced by `uni_dead` for the duration of the call; the module is not edited.  No
element is left out of the metric (attn_core_restatement.ratio): an element whose bound is zero must be exact -- the
probability of every dead pair.  (Rows 0 and L + 1 .. 2L - 1 of dkr are exactly zero in the reference; their bound is the
format's underflow term alone, about 1e-36, and the GPU test asks for exact zeros there separately.)
"""
import contextlib
import os
import sys

import torch
import torch.nn.functional as F

import attn_core_restatement as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import device_rng  # noqa: E402
import t4r_oracle as O  # noqa: E402

MULT, C_EXP = R.MULT, R.C_EXP
GRAD_NAMES = R.GRAD_NAMES["xlnet"]


# ------------------------------------------------------------------------------------------------ the core
def uni_dead(B, L, key_len):
    """[B, 1, L, L] bool: key j of row i is dead when j > i, or when key_len is given and j >= key_len[b] and j != i"""
    i, j = R._ij(L)
    return R_XLNET_DEAD(B, L, key_len) | (j > i)[None, None]


R_XLNET_DEAD = R.xlnet_dead          # the bi rule, bound before any substitution


@contextlib.contextmanager
def _causal_dead_set():
    R.xlnet_dead = uni_dead
    try:
        yield
    finally:
        R.xlnet_dead = R_XLNET_DEAD


def reference(x, key_len=None, mask=None):
    """float64 forward and autograd of the causal core: dict out, lse, prob, dq, dk, dv, dkr, drw, drr (layout of R.reference)"""
    with _causal_dead_set():
        return R.reference("xlnet", x, key_len=key_len, mask=mask)


def bounds(x, ref, key_len=None, mask=None, **kw):
    """per-element bounds of every output of `reference`"""
    with _causal_dead_set():
        return R.bounds("xlnet", x, ref, key_len=key_len, mask=mask, **kw)


# ------------------------------------------------------------------------------------------------ layer and model
def _dead_lm(B, L, key_len, causal):
    dead = torch.zeros(B, 1, L, L, dtype=torch.bool) if key_len is None else O.key_padding_mask(key_len, L)
    if causal:
        i, j = R._ij(L)
        dead = dead | (j > i)[None, None]
    return dead


def rel_attn(h, p, n_head, eps=0.03, causal=False, key_len=None, masks=None, drop_p=0.0):
    """O.xlnet_rel_attn / the attention half of O.xlnet_layer_dropout in the dtype of h, with the causal flag.
    masks: None, or dict pos [B, 2L, D], prob [B, n, L, L], attn_out [B, L, D] of 0 / 1 tensors (training mode)"""
    B, L, D = h.shape
    dh = D // n_head
    s = 1.0 / (1.0 - drop_p)
    q = torch.einsum("blh,hnd->blnd", h, p["q"])
    k = torch.einsum("blh,hnd->blnd", h, p["k"])
    v = torch.einsum("blh,hnd->blnd", h, p["v"])
    pe = O.xlnet_pos_emb(L, D, h.dtype)[None].expand(B, 2 * L, D)
    if masks is not None:
        pe = pe * masks["pos"].to(h.dtype) * s
    k_r = torch.einsum("bph,hnd->bpnd", pe, p["r"])
    ac = torch.einsum("bind,bjnd->bnij", q + p["r_w_bias"], k)
    bd_full = torch.einsum("bind,bpnd->bnip", q + p["r_r_bias"], k_r)
    bd = torch.gather(bd_full, 3, R.shift_index(B, n_head, L))
    score = ((ac + bd) * (1.0 / (dh ** 0.5))).masked_fill(_dead_lm(B, L, key_len, causal), float("-inf"))
    prob = torch.softmax(score, dim=3)
    if masks is not None:
        prob = prob * masks["prob"].to(h.dtype) * s
    av = torch.einsum("bnij,bjnd->bind", prob, v)
    ao = torch.einsum("bind,hnd->bih", av, p["o"])
    if masks is not None:
        ao = ao * masks["attn_out"].to(h.dtype) * s
    return O.layer_norm(ao + h, p["ln_w"], p["ln_b"], eps)


def layer(h, p, n_head, eps=0.03, causal=False, key_len=None, masks=None, drop_p=0.0):
    """one XLNet layer; masks (training mode): the dict of rel_attn plus ff_act [B, L, 4D] and ff_out [B, L, D]"""
    h1 = rel_attn(h, p, n_head, eps, causal, key_len, masks, drop_p)
    if masks is None:
        return O.xlnet_ff(h1, p, eps)
    s = 1.0 / (1.0 - drop_p)
    y = F.gelu(F.linear(h1, p["w1"], p["b1"])) * masks["ff_act"].to(h.dtype) * s
    y = F.linear(y, p["w2"], p["b2"]) * masks["ff_out"].to(h.dtype) * s
    return O.layer_norm(y + h1, p["ff_ln_w"], p["ff_ln_b"], eps)


def model(x, layers, n_head, eps=0.03, causal=False, key_len=None, masks=None, drop_p=0.0):
    """XLNetModel.forward with inputs_embeds only.  masks (training mode): what device_masks returns"""
    if masks is None:
        for p in layers:
            x = layer(x, p, n_head, eps, causal, key_len)
        return x
    s = 1.0 / (1.0 - drop_p)
    h = x * masks["input"].to(x.dtype) * s
    for p, lm in zip(layers, masks["layers"]):
        h = layer(h, p, n_head, eps, causal, key_len, dict(pos=masks["pos"], **lm), drop_p)
    return h * masks["final"].to(x.dtype) * s


def device_masks(B, L, D, n_head, n_layer, p, seed, offset):
    """the keep decisions of one training forward as the device draws them (oracle/device_rng.py): the keys and the 2L-row
    positional layout are those of the bi body"""
    return device_rng.xlnet_dropout_masks(B, L, D, n_head, n_layer, p, seed, offset)


def layer_device_masks(B, L, D, n_head, p, seed, offset, layer_idx):
    """the masks of ONE layer called on its own with (seed, offset, layer_idx): pos is keyed by the model level (255)"""
    ms = device_rng.xlnet_dropout_masks(B, L, D, n_head, layer_idx + 1, p, seed, offset)
    return dict(pos=ms["pos"], **ms["layers"][layer_idx])


def layer_params(g, D, n, scale=0.1, dtype=torch.float32):
    """the 15 tensors of a layer by the oracle's names (order: PARAM_ORDER)"""
    dh = D // n
    r = lambda *s: (scale * torch.randn(*s, generator=g)).to(dtype)
    return dict(q=r(D, n, dh), k=r(D, n, dh), v=r(D, n, dh), o=r(D, n, dh), r=r(D, n, dh), r_w_bias=r(n, dh), r_r_bias=r(n, dh),
                ln_w=1 + r(D), ln_b=r(D), w1=r(4 * D, D), b1=r(4 * D), w2=r(D, 4 * D), b2=r(D), ff_ln_w=1 + r(D), ff_ln_b=r(D))


PARAM_ORDER = ("q", "k", "v", "o", "r", "r_w_bias", "r_r_bias", "ln_w", "ln_b", "w1", "b1", "w2", "b2", "ff_ln_w", "ff_ln_b")
