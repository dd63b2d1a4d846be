"""The attention cores against float64 at the softmax's hard cases, per element (references, bounds and input families:
tests/attn_core_restatement.py, checked without a GPU in tests/test_attn_core_cpu.py, where nine planted faults each leave the
bound on the family named for them).

Compared through the bound: out, lse and every gradient of ops.xlnet_attn_fwd / xlnet_attn_bwd and of ops.mha_fwd / mha_bwd
(fused-row and separate operands), and, where the one-wave matrix-core kernels serve the shape, the stored-probability pair of
include/t4r_hip_attn.h.  Every value is finite; family E is also held to the closed form (mean of v); family Z gives exact
zeros; sessions of family M with key_len >= L are bit-equal to key_len = None.  Every test prints its worst error / bound
(tools/attn_core_margins.py makes profiles/attn_core_margins.txt from them).

Which kernels a shape reaches (the library does not report it; csrc/xlnet_attn.hip attn_uses_long / use_mfma, csrc/mha.hip
mha_short_ok, csrc/mha_mfma.hip t4r_mha_mfma_ok):
    XLNet   L <= 32 and d_head 16 / 32: one-wave matrix-core kernels;  otherwise L <= 64 and d_head 8 / 16 / 32: VALU / LDS
            kernels (pair-decomposed backward for L <= 32);  everything else: the general kernels.
    MHA     L <= 128 and d_head 32 / 64: matrix-core kernels, in BOTH operand layouts (t4r_mha_mfma_ok only wants row strides
            below 2^31 / 160, which 3 D and D both are);  L <= 128 and d_head 16: LDS kernels, both layouts;  else general.
"""
import math

import pytest
import torch

import attn_core_restatement as R
from test_kernels_gpu import ORDER, _mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, F32 = torch.float64, torch.float32
DROP_P, SEED = 0.3, 21


@pytest.fixture(scope="module")
def ops():
    from transformers4rec_amd import ops as o
    return o


def cu(t):
    return t.to(DEV).float().contiguous()


def xlnet_group(L, d):
    return "mfma" if L <= 32 and d in (16, 32) else "valu" if L <= 64 and d in (8, 16, 32) else "general"


def mha_group(L, d):
    return "general" if L > 128 or d not in (16, 32, 64) else "mfma" if d in (32, 64) else "lds"


def drop_of(ops, on, B, n, L):
    """(the kernels' drop argument, the keep decisions times the factor 1 / (1 - p) as fp32 forms it)"""
    if not on:
        return ops.NO_DROP, None
    ctr = ops.dropout_ctr_hi(2, 1, ops.SITE_PROB)
    inv_keep = float(torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(DROP_P, dtype=F32)))
    return (DROP_P, SEED, ctr), _mask(ops, (B, n, L, L), DROP_P, SEED, ctr).double() * inv_keep


class Checks:
    """error / bound of every output of one test over EVERY element: prints each, fails at the end with all misses"""

    def __init__(self, tag):
        self.tag, self.missed = tag, []

    def __call__(self, name, got, ref, bound):
        got = got.double().cpu().reshape(ref.shape)
        if not bool(torch.isfinite(got).all()):
            self.missed.append(f"{name}: not finite")
        r = R.ratio(got, ref, bound)
        print(f"attn_core {self.tag} {name}: worst error / bound {r:.3f}")
        if not r <= 1.0:
            self.missed.append(f"{name}: error / bound {r:.3g}")
        return r

    def done(self):
        assert not self.missed, self.tag + ": " + "; ".join(self.missed)


def smallest_c_exp(tag, kind, x, got, ref, causal, key_len, mask, **kw):
    """family U: the smallest C_EXP that puts every output of this case at <= 0.5 of its bound (how C_EXP was set)"""
    for c in range(0, 65):
        bd = R.bounds(kind, x, ref, causal, key_len, mask, c_exp=c, **kw)
        if all(R.ratio(got[nm].double().cpu(), ref[nm], bd[nm]) <= 0.5 for nm in got):
            print(f"attn_core {tag} smallest C_EXP for 0.5: {c}")
            return
    print(f"attn_core {tag} smallest C_EXP for 0.5: above 64")


def split_case(fam):
    """'U', 'M/U', 'U/drop' -> (family of the inputs, key_len edges?, dropout?)"""
    return fam.split("/")[-1] if fam.startswith("M/") else fam.split("/")[0], fam.startswith("M/"), fam.endswith("/drop")


# ================================================================================================ XLNet relative attention
def run_xlnet(ops, x, B, L, n, d, key_len, drop):
    D = n * d
    f2 = lambda t: cu(t.reshape(-1, D))
    q, k, v, kr, dout = (f2(x[nm]) for nm in ("q", "k", "v", "kr", "dout"))
    rw, rr = cu(x["rw"].reshape(-1)), cu(x["rr"].reshape(-1))
    out, lse = ops.xlnet_attn_fwd(q, k, v, kr, rw, rr, B, L, n, drop=drop, key_len=key_len)
    drw, drr = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    dq, dk, dv, dkr = ops.xlnet_attn_bwd(q, k, v, kr, rw, rr, out, lse, dout, drw, drr, B, L, n, drop=drop, key_len=key_len)
    torch.cuda.synchronize()
    return dict(out=out, lse=lse, dq=dq.clone(), dk=dk.clone(), dv=dv.clone(), dkr=dkr, drw=drw, drr=drr)


def run_xlnet_prob(ops, x, prob, B, L, n, d, drop):
    """the backward that reads the probabilities (include/t4r_hip_attn.h), as tests/test_attn_prob_gpu.py calls it"""
    D = n * d
    f2 = lambda t: cu(t.reshape(-1, D))
    drw, drr = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    dq, dk, dv, dkr = ops.xlnet_attn_bwd_prob(f2(x["q"]), f2(x["k"]), f2(x["v"]), f2(x["kr"]), cu(x["rw"].reshape(-1)),
                                              cu(x["rr"].reshape(-1)), cu(prob), f2(x["dout"]), drw, drr, B, L, n, drop=drop)
    torch.cuda.synchronize()
    return dict(dq=dq.clone(), dk=dk.clone(), dv=dv.clone(), dkr=dkr, drw=drw, drr=drr)


XL_DROP_SHAPES = [(3, 20, 64, 4), (2, 33, 32, 2), (2, 65, 32, 2)]           # dropout once per kernel group, families U and P
XLNET_CASES = ([(s, f) for s in R.XLNET_SHAPES for f in R.FAMILIES + ("M/U", "M/O-")]
               + [(s, f) for s in R.XLNET_STRIDE_SHAPES for f in ("U", "A+")]
               + [(s, f) for s in XL_DROP_SHAPES for f in ("U/drop", "P/drop")])


@pytest.mark.parametrize("shape,fam", XLNET_CASES, ids=lambda z: "x".join(map(str, z)) if isinstance(z, tuple) else z)
def test_xlnet_core(ops, shape, fam):
    B, L, D, n = shape
    d = D // n
    base, masked, dropped = split_case(fam)
    B = 5 if masked else B                                  # family M: one session per key_len edge
    x = R.family(base, B, L, n, d, 0)
    kl = R.mask_edges(L) if masked else None
    kl_dev = kl.to(DEV) if masked else None
    drop, mask = drop_of(ops, dropped, B, n, L)
    ref = R.reference("xlnet", x, key_len=kl, mask=mask)
    bd = R.bounds("xlnet", x, ref, key_len=kl, mask=mask)
    group = xlnet_group(L, d)
    tag = f"xlnet/{group} {fam} B={B} L={L} D={D} n={n}"
    check = Checks(tag)
    got = run_xlnet(ops, x, B, L, n, d, kl_dev, drop)
    for nm in ("out", "lse") + R.GRAD_NAMES["xlnet"]:
        check(nm, got[nm], ref[nm], bd[nm])
    if fam == "U":
        smallest_c_exp(tag, "xlnet", x, got, ref, False, kl, mask)
    if base == "E":                                         # the closed form: p = 1 / L, out = the mean of v
        check("out-vs-mean-of-v", got["out"], x["v"].mean(1, keepdim=True).expand(B, L, n, d), bd["out"])
        assert float((got["lse"].double().cpu() - (R.xlnet_scores(x["q"], x["k"], x["kr"], x["rw"], x["rr"])[..., 0]
                                                   + math.log(L))).abs().max()) <= float(bd["lse"].max())
    if base == "Z1":
        for nm in ("out", "dq", "dk", "dkr", "drw", "drr"):
            assert float(got[nm].abs().max()) == 0.0, f"{tag} {nm}: not exactly zero"
    if masked:                                              # key_len >= L is key_len = None, to the bit (per-session outputs)
        plain = run_xlnet(ops, x, B, L, n, d, None, drop)
        rows = lambda t: t.view(B, -1)[3:]
        for nm in ("out", "lse", "dq", "dk", "dv"):
            assert torch.equal(rows(got[nm]), rows(plain[nm])), f"{tag} {nm}: key_len >= L differs from key_len = None"
        if L > 1:
            assert not torch.equal(got["out"].view(B, -1)[:2], plain["out"].view(B, -1)[:2])
    if group == "mfma" and not masked:                      # the stored-probability backward reads fp64's p, rounded to fp32
        bdp = R.bounds("xlnet", x, ref, mask=mask, p_given=True)
        gp = run_xlnet_prob(ops, x, ref["prob"], B, L, n, d, drop)
        for nm in R.GRAD_NAMES["xlnet"]:
            check("prob-path " + nm, gp[nm], ref[nm], bdp[nm])
        if fam == "U":
            smallest_c_exp(tag + " prob-path", "xlnet", x, gp, ref, False, None, mask, p_given=True)
        if base == "Z1":
            for nm in ("dq", "dk", "dkr", "drw", "drr"):
                assert float(gp[nm].abs().max()) == 0.0, f"{tag} prob-path {nm}: not exactly zero"
    check.done()


# ---- the forward that leaves the probabilities (one-kernel attention block): its core is held from ITS OWN fp32 q | k | v
# the one-wave shapes of R.XLNET_SHAPES that the block kernel takes (d_model 32 / 64 / 128: not (2, 17, 16, 1)), and d_model 128
PROB_FWD_SHAPES = [(3, 20, 64, 4), (2, 32, 64, 2), (2, 1, 32, 2), (3, 17, 64, 4), (3, 20, 128, 4)]


@pytest.mark.parametrize("fam", ["U", "S70", "M/U", "M/S70", "U/drop"])
@pytest.mark.parametrize("B,L,D,n", PROB_FWD_SHAPES)
def test_stored_probabilities_forward(ops, B, L, D, n, fam):
    """t4r_xlnet_attn_block_fwd_prob: prob, lse and the attention vector against the float64 core of the q | k | v the launch
    itself saved (its projections are the subject of tests/test_body_split_gpu.py).  S70: the q projection scaled so that the
    largest |score| is 70 -- the hard cases this entry point can be given, as q, k and v are products of one h"""
    assert ops.xlnet_attn_block_supported(L, D, n)
    base, masked, dropped = split_case(fam)
    B = 5 if masked else B
    d = D // n
    g = torch.Generator().manual_seed(100 * B + L + D)
    r = lambda *s: R.f32(0.15 * torch.randn(*s, generator=g, dtype=F64))
    p = dict(q=r(D, n, d), k=r(D, n, d), v=r(D, n, d), o=r(D, n, d), r=r(D, n, d), r_w_bias=r(n, d), r_r_bias=r(n, d),
             ln_w=1 + r(D), ln_b=r(D), w1=r(4 * D, D), b1=r(4 * D), w2=r(D, 4 * D), b2=r(D), ff_ln_w=1 + r(D), ff_ln_b=r(D))
    h = R.f32(torch.randn(B * L, D, generator=g, dtype=F64))
    kr = R.f32(0.3 * torch.randn(2 * L, n, d, generator=g, dtype=F64))
    if base == "S70":
        proj = lambda w: torch.einsum("bld,dnh->blnh", h.view(B, L, D), w)
        for _ in range(2):
            s = R.xlnet_scores(proj(p["q"]), proj(p["k"]), kr, p["r_w_bias"], p["r_r_bias"])
            p["q"] = R.f32(p["q"] * (70.0 / float(s.abs().max())))
    kl = R.mask_edges(L) if masked else None
    ctr_p = ops.dropout_ctr_hi(5, 1, ops.SITE_PROB)
    planes = ops.xlnet_layer_prepare([cu(p[k]) for k in ORDER], D)
    prob = torch.full((B * n * L * L,), -7.0, device=DEV)
    _, saved = ops.xlnet_attn_block_fwd(cu(h), planes, cu(p["o"]).view(D, D), cu(kr).view(-1, D), cu(p["r_w_bias"]).view(-1),
                                        cu(p["r_r_bias"]).view(-1), cu(p["ln_w"]), cu(p["ln_b"]), B, L, n, 0.03,
                                        DROP_P if dropped else 0.0, SEED, ctr_p, ops.dropout_ctr_hi(5, 1, ops.SITE_ATTN_OUT),
                                        key_len=kl.to(DEV) if masked else None, prob=prob)
    torch.cuda.synchronize()
    x = dict(kr=kr, rw=p["r_w_bias"], rr=p["r_r_bias"], dout=torch.zeros(B, L, n, d, dtype=F64))
    for z, nm in enumerate("qkv"):
        x[nm] = saved["qkv"][z].double().cpu().view(B, L, n, d)
    mask = None
    if dropped:
        inv_keep = float(torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(DROP_P, dtype=F32)))
        mask = _mask(ops, (B, n, L, L), DROP_P, SEED, ctr_p).double() * inv_keep
    ref = R.reference("xlnet", x, key_len=kl, mask=mask)
    bd = R.bounds("xlnet", x, ref, key_len=kl, mask=mask)
    print(f"largest |score| {float(R.xlnet_scores(x['q'], x['k'], kr, x['rw'], x['rr']).abs().max()):.1f}")
    check = Checks(f"xlnet/block-prob {fam} B={B} L={L} D={D} n={n}")
    check("prob", prob.view(B, n, L, L), ref["prob"], bd["prob"])
    check("lse", saved["lse"], ref["lse"], bd["lse"])
    check("out", saved["av"], ref["out"], bd["out"])
    if masked:
        dead = R.xlnet_dead(B, L, kl).expand(B, n, L, L)
        assert bool((prob.view(B, n, L, L).cpu()[dead] == 0).all())
        assert torch.equal(prob.view(B, n, L, L)[0].cpu(), torch.eye(L).expand(n, L, L))      # key_len = 0: the diagonal alone
    check.done()


# ================================================================================================ GPT-2 / BERT attention
def run_mha(ops, x, B, L, n, d, causal, key_len, drop, fused):
    D = n * d
    rows = lambda nm: x[nm].reshape(B * L, D)
    dout = cu(rows("dout"))
    if fused:
        qkv = cu(torch.cat([rows("q"), rows("k"), rows("v")], 1))
        a, b, c = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    else:
        a, b, c = cu(rows("q")), cu(rows("k")), cu(rows("v"))
    out, lse = ops.mha_fwd(a, b, c, B, L, n, causal, drop, key_len=key_len)
    res = ops.mha_bwd(a, b, c, out, lse, dout, B, L, n, causal, drop, fused_out=fused, key_len=key_len)
    torch.cuda.synchronize()
    dq, dk, dv = (res[:, :D], res[:, D:2 * D], res[:, 2 * D:]) if fused else res
    return dict(out=out, lse=lse, dq=dq.contiguous(), dk=dk.contiguous(), dv=dv.contiguous())


MHA_DROP_SHAPES = [(2, 20, 32, 2, True), (2, 33, 64, 1, True), (2, 129, 64, 2, True)]     # LDS, matrix-core, general
MHA_CASES = ([(s, f) for s in R.MHA_SHAPES for f in R.FAMILIES + ("M/U", "M/O-")]
             + [(s, f) for s in MHA_DROP_SHAPES for f in ("U/drop", "P/drop")])


@pytest.mark.parametrize("shape,fam", MHA_CASES, ids=lambda z: "x".join(map(str, z)) if isinstance(z, tuple) else z)
def test_mha_core(ops, shape, fam):
    B, L, D, n, causal = shape
    d = D // n
    base, masked, dropped = split_case(fam)
    B = 5 if masked else B
    x = R.family(base, B, L, n, d, 0, kind="mha")
    kl = R.mask_edges(L) if masked else None
    kl_dev = kl.to(DEV) if masked else None
    drop, mask = drop_of(ops, dropped, B, n, L)
    ref = R.reference("mha", x, causal, kl, mask)
    bd = R.bounds("mha", x, ref, causal, kl, mask)
    tag = f"mha/{mha_group(L, d)} {fam} B={B} L={L} D={D} n={n} causal={int(causal)}"
    check = Checks(tag)
    both = {}
    for fused in (True, False):
        got = both[fused] = run_mha(ops, x, B, L, n, d, causal, kl_dev, drop, fused)
        for nm in ("out", "lse") + R.GRAD_NAMES["mha"]:
            check(("fused " if fused else "separate ") + nm, got[nm], ref[nm], bd[nm])
        if fam == "U":
            smallest_c_exp(tag + (" fused" if fused else " separate"), "mha", x, got, ref, causal, kl, mask)
        if base == "E":                                     # the closed form: the mean of the visible v
            vh = x["v"]
            mean = (vh.cumsum(1) / (torch.arange(L, dtype=F64) + 1).view(1, L, 1, 1)) if causal else vh.mean(1, keepdim=True).expand(B, L, n, d)
            check(("fused " if fused else "separate ") + "out-vs-mean-of-v", got["out"], mean, bd["out"])
        if base == "Z1":
            for nm in ("out", "dq", "dk"):
                assert float(got[nm].abs().max()) == 0.0, f"{tag} {nm}: not exactly zero"
        if masked:                                          # key_len >= L is key_len = None, to the bit
            plain = run_mha(ops, x, B, L, n, d, causal, None, drop, fused)
            for nm in got:
                assert torch.equal(got[nm].view(B, -1)[3:], plain[nm].view(B, -1)[3:]), f"{tag} {nm}: key_len >= L differs from None"
            # key_len = 0 is key_len = 1 (the clamp): session 0 attends to key 0 alone
            assert torch.equal(got["out"].view(B, L, D)[0], cu(x["v"]).view(B, L, D)[0, :1].expand(L, D))
    assert torch.equal(both[True]["out"], both[False]["out"]) and torch.equal(both[True]["lse"], both[False]["lse"])
    check.done()
