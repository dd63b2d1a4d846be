"""The float64 references, error bounds and input families of the attention cores (tests/attn_core_restatement.py), checked
without a GPU on every family and every shape of tests/test_attn_core_gpu.py:
  * the float64 references agree with the references of tests/test_kernels_gpu.py (test_xlnet_attention_core, test_mha_fwd_bwd)
    at unit scale, and their key_len with the oracle's masks (xlnet_rel_attn / key_padding_mask, sdpa) for key_len in [1, L];
  * every family does what its row of the table says (running maximum of A+, one-hot rows of P, overflow / underflow of O+-);
  * an fp32 restatement of the kernels' algorithm (blockwise online softmax, lse = m + log l, a backward that recomputes p from
    lse with D from out) stays at <= 0.5 of the bound everywhere -- the worst ratio is printed;
  * nine planted faults, each a switch on that restatement, each leave the bound (or stop being finite) on the family named
    for them: the evidence that the GPU tests would fail for a subtly wrong kernel.  No kernel is altered for it.
"""
import pytest
import torch

import attn_core_restatement as R
import t4r_oracle as O

F64, F32 = torch.float64, torch.float32
ALL_XLNET = [(s, f) for s in R.XLNET_SHAPES for f in R.FAMILIES] + [(s, f) for s in R.XLNET_STRIDE_SHAPES for f in ("U", "A+")]
ALL_MHA = [(s, f) for s in R.MHA_SHAPES for f in R.FAMILIES]


def _drop_mask(shape, p, seed):
    g = torch.Generator().manual_seed(seed)
    inv_keep = float(torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32)))
    return (torch.rand(shape, generator=g) >= p).to(F64) * inv_keep


# ================================================================================================ the references
@pytest.mark.parametrize("B,L,D,n", [(3, 20, 64, 4), (2, 33, 32, 2), (2, 9, 20, 2)])
def test_xlnet_reference_is_the_existing_one(B, L, D, n):
    """torch.einsum / softmax / autograd exactly as tests/test_kernels_gpu.py::test_xlnet_attention_core writes them"""
    x = R.family("U", B, L, n, D // n, 1)
    q, k, v, kr, rw, rr = (x[nm].clone().requires_grad_() for nm in ("q", "k", "v", "kr", "rw", "rr"))
    dh = D // n
    ac = torch.einsum("bind,bjnd->bnij", q + rw, k)
    bd_full = torch.einsum("bind,pnd->bnip", q + rr, kr)
    idx = torch.arange(L)[None, :] + L - torch.arange(L)[:, None]
    bd = torch.gather(bd_full, 3, idx[None, None].expand(B, n, L, L))
    prob = torch.softmax((ac + bd) / dh ** 0.5, 3)
    out = torch.einsum("bnij,bjnd->bind", prob, v)
    out.backward(x["dout"])
    ref = R.reference("xlnet", x)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-13)
    close(ref["out"], out.detach())
    close(ref["prob"], prob.detach())
    close(ref["lse"], torch.logsumexp((ac + bd).detach() / dh ** 0.5, 3))
    for nm, t in zip(R.GRAD_NAMES["xlnet"], (q, k, v, kr, rw, rr)):
        close(ref[nm], t.grad)


@pytest.mark.parametrize("B,L,D,n,causal", [(2, 20, 32, 2, True), (2, 33, 64, 1, False)])
def test_mha_reference_is_the_existing_one(B, L, D, n, causal):
    """tests/test_kernels_gpu.py::test_mha_fwd_bwd, with a dropout mask"""
    dh = D // n
    x = R.family("U", B, L, n, dh, 2, kind="mha")
    mask = _drop_mask((B, n, L, L), 0.3, 4)
    qkv = torch.cat([x[nm].reshape(B * L, D) for nm in "qkv"], 1).requires_grad_()
    q, k, v = (qkv[:, i * D:(i + 1) * D].view(B, L, n, dh).transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / dh ** 0.5
    if causal:
        s = s.masked_fill(~torch.tril(torch.ones(L, L, dtype=torch.bool)), float("-inf"))
    prob = torch.softmax(s, -1)
    out = ((prob * mask) @ v).transpose(1, 2).reshape(B * L, D)
    out.backward(x["dout"].reshape(B * L, D))
    ref = R.reference("mha", x, causal, mask=mask)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-13)
    close(ref["out"].reshape(B * L, D), out.detach())
    close(ref["prob"], prob.detach())
    close(torch.cat([ref[nm].reshape(B * L, D) for nm in ("dq", "dk", "dv")], 1), qkv.grad)


def test_key_len_is_the_oracles_inside_1_to_L():
    B, L, n, dh = 4, 9, 2, 8
    key_len = torch.tensor([1, 4, 9, 7], dtype=torch.int32)
    assert torch.equal(R.xlnet_dead(B, L, key_len), O.key_padding_mask(key_len, L))
    x = R.family("U", B, L, n, dh, 3)
    # O.xlnet_rel_attn's probabilities (score - 1e30 * mask) with the projections set to pass q, k, v through
    s = R.xlnet_scores(x["q"], x["k"], x["kr"], x["rw"], x["rr"])
    want = torch.softmax(s - 1e30 * O.key_padding_mask(key_len, L).to(F64), 3)
    torch.testing.assert_close(R.xlnet_core(x["q"], x["k"], x["v"], x["kr"], x["rw"], x["rr"], key_len)[2], want, rtol=1e-12, atol=1e-15)
    D = n * dh
    f = lambda t: t.reshape(B, L, D)
    for causal in (False, True):
        want = O.sdpa(f(x["q"]), f(x["k"]), f(x["v"]), n, causal, key_len)
        torch.testing.assert_close(f(R.mha_core(x["q"], x["k"], x["v"], causal, key_len)[0]), want, rtol=1e-12, atol=1e-14)


def test_key_len_outside_1_to_L():
    """the kernels' stated conventions: MHA clamps to [1, L]; XLNet keeps the diagonal, so 0 is self-attention and > L unmasked"""
    B, L, n, dh = 5, 6, 1, 4
    x = R.family("U", B, L, n, dh, 4)
    kl = R.mask_edges(L)
    out, lse, prob = R.xlnet_core(x["q"], x["k"], x["v"], x["kr"], x["rw"], x["rr"], kl)
    assert torch.equal(prob[0, 0], torch.eye(L, dtype=F64)) and torch.equal(out[0], x["v"][0])
    full = R.xlnet_core(x["q"], x["k"], x["v"], x["kr"], x["rw"], x["rr"])
    assert torch.equal(out[3:], full[0][3:]) and torch.equal(lse[3:], full[1][3:])
    for causal in (False, True):
        got = R.mha_core(x["q"], x["k"], x["v"], causal, kl)
        same = R.mha_core(x["q"], x["k"], x["v"], causal, torch.tensor([1, 1, 3, 6, 6]))
        assert all(torch.equal(a, b) for a, b in zip(got, same))


# ================================================================================================ the families
@pytest.mark.parametrize("shape", R.XLNET_SHAPES + R.XLNET_STRIDE_SHAPES + R.MHA_SHAPES)
def test_families_do_what_their_row_says(shape):
    kind, causal = ("mha", shape[4]) if len(shape) == 5 else ("xlnet", False)
    B, L, D, n = shape[:4]
    dead = (R.mha_dead(B, L, causal, None) if kind == "mha" else R.xlnet_dead(B, L, None)).expand(B, n, L, L)
    visible = (~dead).sum(3)
    sc = lambda x: R._scores_of(kind, x)
    for name in ("A+", "A-"):
        ch = R.running_max_changes(sc(R.family(name, B, L, n, D // n, 0, kind)), dead)
        if name == "A+":
            assert bool((ch >= visible - 1).all()), "A+: the running maximum must rise at every key"
        else:
            assert bool((ch == 1).all()), "A-: the running maximum must never rise after the first key"
    if len(shape) == 4 and shape in R.XLNET_STRIDE_SHAPES:
        return
    x = R.family("P", B, L, n, D // n, 0, kind)
    s = sc(x)
    assert 60.0 <= float(s.abs().max()) <= 80.0
    frac = R.peaked_fraction(R.reference(kind, x, causal)["prob"])
    print(f"P {shape}: top probability >= 0.99 in {100 * frac:.1f} % of the rows")
    assert frac >= 0.9
    for name, sign in (("O+", 1), ("O-", -1)):
        s = sc(R.family(name, B, L, n, D // n, 0, kind))
        assert float((s - R.O_TARGET[name]).abs().max()) <= 2.0
        assert R.naive_exp_fails(s, dead, sign)
    p = R.reference(kind, R.family("E", B, L, n, D // n, 0, kind), causal)["prob"]
    assert float((p - torch.where(dead, torch.zeros_like(p), 1.0 / visible[..., None].to(F64))).abs().max()) < 1e-15


# ================================================================================================ the fp32 restatement
def _cases():
    for (B, L, D, n), fam in ALL_XLNET:
        yield "xlnet", (B, L, D, n), fam, False
    for (B, L, D, n, causal), fam in ALL_MHA:
        yield "mha", (B, L, D, n), fam, causal


@pytest.fixture(scope="module")
def worst():
    """{(kind, family): {output: worst ratio over the shapes}} of the unfaulted fp32 restatement, C_EXP = 0; M on U and O-"""
    table = {}

    def add(kind, fam, r):
        slot = table.setdefault((kind, fam), {})
        for nm, val in r.items():
            slot[nm] = max(slot.get(nm, 0.0), val)
    for kind, (B, L, D, n), fam, causal in _cases():
        x = R.family(fam, B, L, n, D // n, 0, kind)
        mask = _drop_mask((B, n, L, L), 0.3, L) if fam in ("U", "P") and B <= 3 else None
        for mk in ((None, mask) if mask is not None else (None,)):
            ref = R.reference(kind, x, causal, mask=mk)
            add(kind, fam, R.worst_ratios(kind, x, R.restated(kind, x, causal, mask=mk, block=16 if L > 16 else 4), ref=ref,
                                          bd=R.bounds(kind, x, ref, causal, mask=mk, c_exp=0)))
            if kind == "xlnet" and L <= 32 and D // n in (16, 32):       # the backward that reads the probabilities
                got = R.restated(kind, x, mask=mk, prob=ref["prob"])
                r = R.worst_ratios(kind, x, {nm: got[nm] for nm in R.GRAD_NAMES[kind]}, ref=ref,
                                   bd=R.bounds(kind, x, ref, mask=mk, c_exp=0, p_given=True))
                add(kind, fam, {"prob-path " + nm: val for nm, val in r.items()})
        if fam in ("U", "O-") and B <= 3:
            xm = R.family(fam, 5, L, n, D // n, 0, kind)
            kl = R.mask_edges(L)
            add(kind, "M/" + fam, R.worst_ratios(kind, xm, R.restated(kind, xm, causal, kl), causal, kl, c_exp=0))
    return table


def test_fp32_restatement_stays_inside_half_the_bound(worst):
    top = 0.0
    for (kind, fam), slot in sorted(worst.items()):
        print(f"{kind:5s} {fam:5s} " + "  ".join(f"{nm} {val:.3f}" for nm, val in slot.items()))
        top = max(top, max(slot.values()))
    print(f"worst error / bound of the fp32 restatement with C_EXP = 0 and MULT = {R.MULT}: {top:.3f}")
    assert top <= 0.5


# (fault, family that must catch it, kind, (B, L, D, n), causal, key_len of family M or None)
PLANTED = [(1, "O+", "xlnet", (2, 33, 32, 2), False, False), (1, "O-", "mha", (2, 33, 64, 1), True, False),
           (2, "A+", "xlnet", (2, 65, 32, 2), False, False), (2, "A+", "mha", (2, 20, 32, 2), True, False),
           (3, "P", "xlnet", (3, 20, 64, 4), False, False), (3, "P", "mha", (2, 20, 32, 2), True, False),
           (4, "E", "xlnet", (3, 20, 64, 4), False, False), (4, "E", "mha", (2, 20, 32, 2), False, False),
           (5, "A-", "xlnet", (2, 20, 16, 2), False, False), (5, "A-", "mha", (2, 33, 64, 1), True, False),
           (6, "O-", "xlnet", (2, 20, 16, 2), False, True),
           (7, "U", "mha", (2, 20, 32, 2), False, True),
           (8, "Z1", "mha", (2, 20, 32, 2), True, False), (8, "Z2", "mha", (2, 7, 64, 1), True, False),
           (9, "U", "xlnet", (3, 20, 64, 4), False, True), (9, "O-", "xlnet", (2, 65, 32, 2), False, True)]


@pytest.mark.parametrize("fault,fam,kind,shape,causal,masked", PLANTED)
def test_planted_fault_leaves_the_bound(fault, fam, kind, shape, causal, masked):
    """with `masked` the catcher is family M (key_len edges) on top of `fam`"""
    B, L, D, n = shape
    B = 5 if masked else B
    x = R.family(fam, B, L, n, D // n, 0, kind)
    kl = R.mask_edges(L) if masked else None
    block = 16 if L > 16 else 4
    ref = R.reference(kind, x, causal, kl)
    bd = R.bounds(kind, x, ref, causal, kl)
    clean = R.worst_ratios(kind, x, R.restated(kind, x, causal, kl, block=block), ref=ref, bd=bd)
    bad = R.worst_ratios(kind, x, R.restated(kind, x, causal, kl, block=block, fault=fault), ref=ref, bd=bd)
    print(f"fault {fault} ({R.FAULTS[fault]}) on {'M/' if masked else ''}{fam} {kind} {shape}: worst error / bound "
          f"{max(bad.values()):.3g} in {max(bad, key=bad.get)} (unfaulted {max(clean.values()):.3f})")
    assert max(clean.values()) <= 1.0
    assert max(bad.values()) > 1.0


def test_every_family_but_U_is_a_named_catcher():
    named = {("M" if masked else fam[0] + fam[1:].strip("12")) for _, fam, _, _, _, masked in PLANTED}
    assert named >= {"P", "A+", "A-", "O+", "O-", "E", "M", "Z"} and {f for f, *_ in PLANTED} == set(R.FAULTS)
