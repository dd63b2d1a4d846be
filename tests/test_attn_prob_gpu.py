"""The attention probabilities handed from the one-kernel forward to the core's backward (include/t4r_hip_attn.h):
  * t4r_xlnet_attn_block_fwd_prob stores P = softmax_j((ac + bd) d_head^-0.5) BEFORE dropout, [B][n_head][L][L], and changes
    no bit of anything else it writes;
  * t4r_xlnet_attn_bwd_prob reads P instead of recomputing the scores, with the contractions over sequence positions cut to
    the session length (csrc/xlnet_attn_mfma.hip: HAVE_P, KH = 8 / 10 / 12 / 16 for L <= 16 / 20 / 24 / 32).
References are fp64 restatements of HF modeling_xlnet.py rel_attn_core :96-140 with rel_shift_bnij :86-94 and their autograd.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ORDER = ("q", "k", "v", "o", "r", "r_w_bias", "r_r_bias", "ln_w", "ln_b", "w1", "b1", "w2", "b2", "ff_ln_w", "ff_ln_b")
SEED, CTR_P, CTR_O = 1234, (5 << 16) | (1 << 8) | 2, (5 << 16) | (1 << 8) | 3
MARGIN, POISON = 64, 7777.0          # floats on either side of the P buffer (a multiple of 4: the buffer stays 16-byte aligned)


@pytest.fixture(scope="module")
def ops():
    from transformers4rec_amd import ops as o
    return o


def cu(t):
    return t.to(DEV).float().contiguous()


def _mask(ops, shape, p, seed, ctr):
    n = int(np.prod(shape))
    _, m = ops.dropout(torch.ones(1, device=DEV), p, seed, ctr, n_total=n, want_mask=True)
    return m.view(shape).double().cpu() / (1.0 - p)


def _scores(q, k, kr, rw, rr, key_len):
    """q, k [B, L, n, dh]; kr [2L, n, dh] or [B, 2L, n, dh]; -> masked scaled scores [B, n, L, L] (fp64 in, fp64 out)"""
    B, L, n, dh = q.shape
    ac = torch.einsum("bind,bjnd->bnij", q + rw, k)
    raw = torch.einsum("bind,bpnd->bnip" if kr.dim() == 4 else "bind,pnd->bnip", q + rr, kr)
    i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
    bd = torch.gather(raw, 3, (j + L - i).expand(B, n, L, L))
    s = (ac + bd) / math.sqrt(dh)
    if key_len is not None:
        dead = (j[None] >= key_len.long().view(B, 1, 1)) & (j != i)[None]
        s = s.masked_fill(dead[:, None], float("-inf"))
    return s


# ------------------------------------------------------------------------------------------------------------ forward
def _block_inputs(ops, B, L, D, n, with_len):
    g = torch.Generator().manual_seed(100 * B + L + D)
    dh = D // n
    r = lambda *s: (0.15 * torch.randn(*s, generator=g, dtype=torch.float64)).float().double()
    p = dict(q=r(D, n, dh), k=r(D, n, dh), v=r(D, n, dh), o=r(D, n, dh), r=r(D, n, dh), r_w_bias=r(n, dh), r_r_bias=r(n, dh),
             ln_w=1 + r(D), ln_b=r(D), w1=r(4 * D, D), b1=r(4 * D), w2=r(D, 4 * D), b2=r(D), ff_ln_w=1 + r(D), ff_ln_b=r(D))
    h = torch.randn(B * L, D, generator=g, dtype=torch.float64).float().double()
    kr = (0.3 * torch.randn(B, 2 * L, D, generator=g, dtype=torch.float64)).float().double()        # per session, for every p
    key_len = torch.randint(1, L + 1, (B,), generator=g) if with_len else None
    planes = ops.xlnet_layer_prepare([cu(p[k]) for k in ORDER], D)
    return p, h, kr, key_len, planes


@pytest.mark.parametrize("with_len", [False, True])
@pytest.mark.parametrize("drop_p", [0.0, 0.3])
@pytest.mark.parametrize("B,L,n,dh", [(3, 20, 4, 32), (3, 17, 4, 16), (2, 32, 2, 32)])
def test_forward_leaves_the_probabilities(ops, B, L, n, dh, drop_p, with_len):
    D = n * dh
    assert ops.xlnet_attn_block_supported(L, D, n)
    p, h, kr, key_len, planes = _block_inputs(ops, B, L, D, n, with_len)
    kl = None if key_len is None else key_len.to(DEV).to(torch.int32)
    N = B * n * L * L

    def run(pd, with_prob):
        buf = torch.full((MARGIN + N + MARGIN,), POISON, device=DEV)
        h1, saved = ops.xlnet_attn_block_fwd(cu(h), planes, cu(p["o"]).view(D, D), cu(kr).view(-1, D), cu(p["r_w_bias"]).view(-1),
                                              cu(p["r_r_bias"]).view(-1), cu(p["ln_w"]), cu(p["ln_b"]), B, L, n, 0.03, pd, SEED,
                                              CTR_P, CTR_O, key_len=kl, prob=buf[MARGIN:MARGIN + N] if with_prob else None)
        torch.cuda.synchronize()
        return h1, saved, buf

    h1, saved, buf = run(drop_p, True)
    # the margins are intact, and so is a buffer that was not handed over
    assert bool((buf[:MARGIN] == POISON).all()) and bool((buf[MARGIN + N:] == POISON).all())
    h1n, savedn, bufn = run(drop_p, False)
    assert bool((bufn == POISON).all())
    # everything else the forward writes is bit-identical with and without the pointer
    assert torch.equal(h1, h1n)
    for name in ("av", "lse", "ao", "qkv", "mean", "rstd"):
        assert torch.equal(saved[name], savedn[name]), name
    P = buf[MARGIN:MARGIN + N].view(B, n, L, L).double().cpu()
    assert bool(((P >= 0) & (P <= 1)).all())                     # every element was written (none is the poison)
    # fp64 softmax of the reference scores, at the forward tolerance of tests/test_attn_block_gpu.py (6e-6 of the largest value)
    hb = h.view(B, L, D)
    q = torch.einsum("bld,dnh->blnh", hb, p["q"])
    k = torch.einsum("bld,dnh->blnh", hb, p["k"])
    s = _scores(q, k, kr.view(B, 2 * L, n, dh), p["r_w_bias"], p["r_r_bias"], key_len)
    Pref = torch.softmax(s, dim=-1)
    print(f"max |P - ref| = {float((P - Pref).abs().max()):.3e}; max |row sum - 1| = {float((P.sum(-1) - 1).abs().max()):.3e}")
    assert float((P - Pref).abs().max()) / float(Pref.abs().max()) < 6e-6
    # rows sum to 1: at most 32 fp32 terms, each within a few ulp (exp, one division) of its exact value
    assert float((P.sum(-1) - 1).abs().max()) < 1e-5
    # exact zeros at masked columns
    if key_len is not None:
        assert bool((P[torch.isinf(s)] == 0).all()) and bool(torch.isinf(s).any())
    # the probabilities are those BEFORE dropout: the same bits at p = 0
    if drop_p > 0:
        _, _, buf0 = run(0.0, True)
        assert torch.equal(buf0, buf)


# ----------------------------------------------------------------------------------------------------------- backward
# (B, L, n, d_head): the forward's shapes, then L = 21, 24, 1 (KH = 12, 12, 8) and the session loop past the 1024-workgroup grid
BWD_SHAPES = [(3, 20, 4, 32), (3, 17, 4, 16), (2, 32, 2, 32), (3, 21, 2, 32), (2, 24, 4, 16), (3, 1, 2, 16), (1030, 20, 4, 32)]
# (dropout p, per-session k_r, key_len)
BWD_MODES = [(0.0, False, False), (0.3, True, False), (0.3, False, True), (0.0, True, True)]


def _bwd_case(ops, B, L, n, dh, p, per_session, klen):
    """inputs and the fp64 autograd reference of one case"""
    g = torch.Generator().manual_seed(B + 3 * L + n * dh)
    D = n * dh
    seed, ctr = 5, ops.dropout_ctr_hi(4, 2, ops.SITE_PROB)
    rnd = lambda *s: torch.randn(*s, generator=g).double()
    q, k, v = (rnd(B, L, n, dh).requires_grad_() for _ in range(3))
    kr = rnd(*((B,) if per_session else ()), 2 * L, n, dh).requires_grad_()
    rw, rr = (0.5 * rnd(n, dh)).requires_grad_(), (0.5 * rnd(n, dh)).requires_grad_()
    key_len = torch.randint(1, L + 1, (B,), generator=g, dtype=torch.int32) if klen else None
    m = _mask(ops, (B, n, L, L), p, seed, ctr) if p > 0 else torch.ones(B, n, L, L, dtype=torch.float64)
    prob = torch.softmax(_scores(q, k, kr, rw, rr, key_len), 3)
    ref = torch.einsum("bnij,bjnd->bind", prob * m, v)
    dout = rnd(B, L, n, dh)
    ref.backward(dout)
    f2 = lambda t: t.detach().reshape(-1, D).float().to(DEV).contiguous()
    want = [t.grad.reshape(-1, D) for t in (q, k, v, kr)] + [rw.grad.reshape(-1), rr.grad.reshape(-1)]
    case = dict(q=f2(q), k=f2(k), v=f2(v), kr=f2(kr), rw=f2(rw).reshape(-1), rr=f2(rr).reshape(-1), dout=f2(dout),
                prob=prob.detach().float().to(DEV).contiguous(), key_len=key_len.to(DEV) if klen else None,
                drop=(p, seed, ctr) if p > 0 else ops.NO_DROP, want=want)
    return case


# tolerances of tests/test_kernels_gpu.py::test_xlnet_attention_core (its `close`: rtol 2e-5 and these atol)
ATOL = dict(dq=1e-4, dk=1e-4, dv=1e-4, dkr=2e-4, drw=3e-4, drr=3e-4)
NAMES = ("dq", "dk", "dv", "dkr", "drw", "drr")


def _run_prob(ops, c, B, L, n):
    D = c["q"].shape[1]
    drw, drr = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    dq, dk, dv, dkr = ops.xlnet_attn_bwd_prob(c["q"], c["k"], c["v"], c["kr"], c["rw"], c["rr"], c["prob"], c["dout"], drw, drr,
                                              B, L, n, drop=c["drop"])
    return [t.clone() for t in (dq, dk, dv, dkr, drw, drr)]


@pytest.mark.parametrize("p,per_session,klen", BWD_MODES)
@pytest.mark.parametrize("B,L,n,dh", BWD_SHAPES)
def test_backward_reads_the_probabilities(ops, B, L, n, dh, p, per_session, klen):
    c = _bwd_case(ops, B, L, n, dh, p, per_session, klen)
    got = _run_prob(ops, c, B, L, n)
    for name, gt, wt in zip(NAMES, got, c["want"]):
        err = float((gt.double().cpu() - wt).abs().max())
        print(f"{name}: max |err| {err:.3e} (largest |value| {float(wt.abs().max()):.3e})")
    for name, gt, wt in zip(NAMES, got, c["want"]):
        torch.testing.assert_close(gt.cpu(), wt.float(), rtol=2e-5, atol=ATOL[name], msg=lambda m, name=name: f"{name}: {m}")
    # run to run: the same bits
    again = _run_prob(ops, c, B, L, n)
    for name, a, b in zip(NAMES, got, again):
        assert torch.equal(a, b), name
    # the recomputing path (t4r_xlnet_attn_bwd after t4r_xlnet_attn_fwd) agrees within the same tolerance
    out, lse = ops.xlnet_attn_fwd(c["q"], c["k"], c["v"], c["kr"], c["rw"], c["rr"], B, L, n, drop=c["drop"], key_len=c["key_len"])
    D = n * dh
    drw, drr = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    dq, dk, dv, dkr = ops.xlnet_attn_bwd(c["q"], c["k"], c["v"], c["kr"], c["rw"], c["rr"], out, lse, c["dout"], drw, drr, B, L, n,
                                         drop=c["drop"], key_len=c["key_len"])
    for name, a, b in zip(NAMES, got, (dq, dk, dv, dkr, drw, drr)):
        torch.testing.assert_close(a.cpu(), b.cpu(), rtol=2e-5, atol=ATOL[name], msg=lambda m, name=name: f"P path vs recompute, {name}: {m}")


def test_backward_argument_errors(ops):
    from transformers4rec_amd import _lib
    z = torch.zeros(2 * 40 * 64, device=DEV)
    with pytest.raises(_lib.T4RHipError, match="one-wave kernels only"):           # L > 32 has no kernel that reads P
        ops.xlnet_attn_bwd_prob(z.view(-1, 64), z.view(-1, 64), z.view(-1, 64), z.view(-1, 64), z[:64], z[:64], z, z.view(-1, 64),
                                z[:64].clone(), z[:64].clone(), 2, 40, 2)
