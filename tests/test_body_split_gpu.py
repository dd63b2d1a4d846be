"""The two-way fp16 split of the XLNet body against fp64 at every magnitude, per row (budget and input families:
tests/body_split_restatement.py, checked without a GPU in tests/test_body_split_cpu.py).

What each family would catch if the scale policy behind it broke:
  A  global magnitudes        a scale that is not applied (or applied twice) on the way out, an overflowing product of scales
  B  per-row magnitudes       a row scale shared by a tile or a tensor (rows 2^-20 and more below a neighbour go under ITS
                              floor), a zero row's scale (pow2_scale(0) = 1, no 0 * inf), a ragged tile's clamped rows
  C  in-row range             the 2^16 .. 2^17 window (full bound inside it) and the floor below it (finite, floor-sized error)
  D  loose activation bound   the a-priori bounds of the FF activation / d pre rows, the keep factor inside them
  E  zero operand             exact zeros where the mathematics gives zeros, no NaN from a zero maximum
  stale maxima                the producer-written operand maxima of the weight-gradient GEMMs: slots of an earlier call, of
                              another grid, or of a row-mapped launch's compact tiles must not reach the next call
Two metrics: the tensor-relative error max |err| / max |ref| at the limits tests/test_fused_gpu.py asserts at unit scale, and
the per-row error against the restatement's bound.  Every test prints its worst error / bound.  Where a quantity is not
homogeneous in its inputs (d pre through GELU', everything behind a softmax whose scores exceed 100) the restatement's docstring
derives what is asserted instead."""
import math

import pytest
import torch

import body_split_restatement as R
import t4r_oracle as O
from test_attn_block_gpu import reference as attn_reference
from test_fused_gpu import ORDER, _mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, F32 = torch.float64, torch.float32
EPS = 0.03
SEED, CTR_A, CTR_O = 99, 4004, 5005


@pytest.fixture(scope="module")
def ops():
    from transformers4rec_amd import ops as o
    return o


def cu(t):
    return t.to(DEV).float().contiguous()


def c64(t):
    return t.double().cpu()


def inv_keep_of(p):
    """1 / (1 - p) as the kernels form it (fp32)"""
    return float(torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))) if p > 0 else 1.0


def mask(ops, shape, p, seed, ctr):
    """the device's keep decisions times the device's factor; ones without dropout"""
    if p == 0:
        return torch.ones(shape, dtype=F64)
    return _mask(ops, shape, p, seed, ctr) * (1.0 - p) * inv_keep_of(p)


def other_params(g, D, n=2, scale=0.1):
    dh = D // n
    r = lambda *s: R.f32(scale * torch.randn(*s, generator=g, dtype=F64))
    return dict(q=r(D, n, dh), k=r(D, n, dh), v=r(D, n, dh), o=r(D, n, dh), r=r(D, n, dh), r_w_bias=r(n, dh), r_r_bias=r(n, dh),
                ln_w=R.f32(1 + r(D)), ln_b=r(D))


class Checks:
    """both metrics of the module docstring for every output of one test: prints each margin, fails at the end with all misses"""

    def __init__(self):
        self.missed = []

    def __call__(self, label, got, ref, bound=None, rel=None):
        got = c64(got)
        assert bool(torch.isfinite(got).all()), f"{label}: not finite"
        msg = f"{label}:"
        if rel is not None:
            e = R.tensor_rel(got, ref)
            msg += f" tensor-relative error {e:.2e} (limit {rel:.0e})"
            if not e < rel:
                self.missed.append(f"{label}: tensor-relative error {e:.3e} >= {rel:.0e}")
        if bound is not None:
            ratio, left = R.row_ratio(got, ref, bound)
            msg += f" worst error / bound {ratio:.3f} ({left} rows left out)"
            if not ratio <= 1.0:
                self.missed.append(f"{label}: error / bound {ratio:.3g}")
        print(msg)

    def done(self):
        assert not self.missed, "; ".join(self.missed)


# ================================================================================================ feed-forward pair
FF_CASES = [(T, D, f) for T, D in ((37, 32), (37, 64), (37, 128)) for f in R.FF_FAMILIES] + [(4099, 64, "B"), (12413, 128, "B")]


@pytest.mark.parametrize("T,D,name", FF_CASES)
def test_ff_pair_every_magnitude(ops, T, D, name):
    h1, p, dy, drop_p = R.ff_family(name, T, D)
    full = dict(other_params(torch.Generator().manual_seed(D), D), **p)
    prm = [cu(full[k]) for k in ORDER]
    planes = ops.xlnet_layer_prepare(prm, D)
    ma, mo = mask(ops, (T, 4 * D), drop_p, SEED, CTR_A), mask(ops, (T, D), drop_p, SEED, CTR_O)
    ref = R.ff_chain(R.Exact(F64), h1, p, dy, ma, mo, EPS)
    bd = R.ff_bounds(ref, h1, p, dy, ma, mo, inv_keep_of(drop_p), EPS)
    fwd = lambda: ops.xlnet_ff_fwd(cu(h1), planes, prm[10], prm[12], prm[13], prm[14], EPS, drop_p, SEED, CTR_A, CTR_O)
    hout, sv = fwd()
    tag, check = f"ff {name} T={T} D={D}", Checks()
    check(f"{tag} ffpre", sv["ffpre"], ref["ffpre"], bd["ffpre"], 3e-6)
    check(f"{tag} ffact", sv["ffact"], ref["ffact"], bd["ffact"], 3e-6)
    check(f"{tag} ffout", sv["ffout"], ref["ffout"], bd["ffout"], 5e-6)
    check(f"{tag} hout", hout, ref["hout"], bd["hout"], 1e-5)
    check(f"{tag} mean", sv["mean"].view(T, 1), ref["mean"], bd["mean"])            # a cancelling sum: per row, on the row's max |x|
    check(f"{tag} rstd", sv["rstd"].view(T, 1), ref["rstd"], bd["rstd"], 1e-5)      # what scales hout: hout's limit
    hout2, sv2 = fwd()
    assert torch.equal(hout, hout2) and all(torch.equal(sv[k], sv2[k]) for k in sv)

    def bwd():
        z = lambda k: torch.zeros(k, device=DEV)
        dg, db, db2, db1 = z(D), z(D), z(D), z(4 * D)
        out = ops.xlnet_ff_bwd(cu(dy), cu(h1), sv, prm[13], planes, dg, db, db2, db1, drop_p, SEED, CTR_A, CTR_O)
        return out + (dg, db, db2, db1)
    dh1, dffout, dpre, dg, db, db2, db1 = bwd()
    check(f"{tag} dffout", dffout, ref["dffout"], bd["dffout"])      # the two row operands: per row (d pre = d act gelu'(pre)
    check(f"{tag} dpre", dpre, ref["dpre"], bd["dpre"])              # is not homogeneous in pre: its bound carries 0.8 e_pre |d act|)
    check(f"{tag} dh1", dh1, ref["dh1"], bd["dh1"], 3e-5)
    for k, t in (("d_b1", db1), ("d_b2", db2), ("d_ff_ln_w", dg), ("d_ff_ln_b", db)):
        check(f"{tag} {k}", t.view(1, -1), ref[k].view(1, -1), None, 3e-5)
    # the rows the two weight gradients contract over
    check(f"{tag} d_w2_rows", c64(dffout).t() @ ref["ffact"], ref["d_w2"], None, 3e-5)
    check(f"{tag} d_w1_rows", c64(dpre).t() @ h1, ref["d_w1"], None, 3e-5)
    again = bwd()
    assert all(torch.equal(a, b) for a, b in zip((dh1, dffout, dpre, dg, db, db2, db1), again))
    # exact zeros where the mathematics gives zeros
    zero_dy = (dy == 0).all(dim=1)
    if bool(zero_dy.any()):
        for t in (dffout, dpre, dh1):
            assert float(c64(t)[zero_dy].abs().max()) == 0.0
    if name == "Etok":
        assert torch.equal(c64(sv["ffpre"]), p["b1"].expand(T, -1))
    if name == "Edy":
        assert all(float(t.abs().max()) == 0.0 for t in (dh1, dffout, dpre, dg, db, db2, db1))
    if name == "Ew2":
        assert torch.equal(c64(sv["ffout"]), p["b2"].expand(T, -1))
        assert float(dpre.abs().max()) == 0.0 and float(db1.abs().max()) == 0.0
    check.done()


# ================================================================================================ projections around attention
PROJ_FAMILIES = ["A0", "A1", "A2", "A3", "A4", "B", "Etok", "Edy", "Eweight"]


def proj_family(name, T, D, seed):
    """token rows x [T, D] (a second operand y and an upstream gradient dy drawn alike), weight factor sw"""
    g = torch.Generator().manual_seed(100 * seed + T + D + 17 * PROJ_FAMILIES.index(name))
    x, y, dy = (torch.randn(T, D, generator=g, dtype=F64) for _ in range(3))
    sw = 1.0
    if name[0] == "A":
        sx, sw, sg = R.A_GRID[int(name[1])]
        x, y, dy = x * sx, y * sx, dy * sg
    elif name == "B":
        e = R.row_exponents(T, g)
        x, y, dy = x * e, y * e, dy * R.row_exponents(T, g) * R.mlm_rows(T, g)
    elif name == "Etok":
        x, y = torch.zeros_like(x), torch.zeros_like(y)
    elif name == "Edy":
        dy = torch.zeros_like(dy)
    elif name == "Eweight":
        sw = 0.0
    return R.f32(x), R.f32(y), R.f32(dy), sw, g


def row_scale(a):
    return R.pow2_scale(R.row_amax(a.to(F32)))


PROJ_CASES = [(T, D, f) for T, D in ((37, 32), (37, 128)) for f in PROJ_FAMILIES]


@pytest.mark.parametrize("T,D,name", PROJ_CASES)
def test_qkv_kr_dh_every_magnitude(ops, T, D, name):
    x, _, dy, sw, g = proj_family(name, T, D, 1)
    p = other_params(g, D)
    for k in ("q", "k", "v", "r"):
        p[k] = R.f32(p[k] * sw)
    full = dict(R.ff_params(g, D), **p)
    planes = ops.xlnet_layer_prepare([cu(R.f32(full[k])) for k in ORDER], D)
    tag, check = f"proj {name} T={T} D={D}", Checks()
    qkv = ops.xlnet_qkv_proj(cu(x), planes)
    for z, nm in enumerate("qkv"):
        w = p[nm].reshape(D, D)
        check(f"{tag} {nm}", qkv[z], x @ w, R.split_bound(x, w, row_scale(x), R.matrix_scale(w.float())) + R.U * (x @ w).abs(), 3e-6)
    w = p["r"].reshape(D, D)
    check(f"{tag} k_r", ops.xlnet_kr_proj(cu(x), planes), x @ w, R.split_bound(x, w, row_scale(x), R.matrix_scale(w.float())), 3e-6)
    # d h = base + sum_z d z @ W_z^T: three products, each row of each gradient with its own scale
    dz = [dy, R.f32(dy.flip(0) * 2.0 ** -7), R.f32(dy.roll(3, 0) * 2.0 ** 9)]
    base = R.f32(torch.randn(T, D, generator=g, dtype=F64) * (1.0 if name == "Edy" else dy.abs().amax(1, keepdim=True)))
    ref, bound, size = base.clone(), torch.zeros(T, D, dtype=F64), base.abs()
    for z, nm in enumerate("qkv"):
        w = p[nm].reshape(D, D).t()
        ref = ref + dz[z] @ w
        size = size + dz[z].abs() @ w.abs()
        bound = bound + R.split_bound(dz[z], w, row_scale(dz[z]), R.matrix_scale(w.float()))
    dh = ops.xlnet_dh_(cu(torch.stack(dz)), planes, cu(base))
    check(f"{tag} dh", dh, ref, bound + 4 * R.U * size, 3e-6)
    if name in ("Etok", "Eweight"):
        assert float(qkv.abs().max()) == 0.0
    if name in ("Eweight", "Edy"):          # all-zero weights, or all-zero d q | d k | d v: d h is the base, bit for bit
        assert torch.equal(c64(dh), base)
    check.done()


@pytest.mark.parametrize("drop_p", [0.0, 0.3])
@pytest.mark.parametrize("T,D,name", PROJ_CASES)
def test_oproj_ln_and_ln1_bwd_every_magnitude(ops, T, D, name, drop_p):
    av, h, dy, sw, g = proj_family(name, T, D, 2)
    p = other_params(g, D)
    p["o"] = R.f32(p["o"] * sw)
    full = dict(R.ff_params(g, D), **p)
    planes = ops.xlnet_layer_prepare([cu(R.f32(full[k])) for k in ORDER], D)
    gam, bet, wo = p["ln_w"], p["ln_b"], p["o"].reshape(D, D)
    m = mask(ops, (T, D), drop_p, SEED, CTR_O)
    drop = (drop_p, SEED, CTR_O) if drop_p > 0 else ops.NO_DROP
    s_o = R.matrix_scale(wo.float())
    ao = av @ wo.t()
    x = ao * m + h
    mu, rs, xh = R.ln_stats(x, EPS)
    e_ao = R.split_bound(av, wo.t(), row_scale(av), s_o)
    e_x = m * e_ao + R.U * x.abs()
    tag, check = f"oproj {name} T={T} D={D} p={drop_p}", Checks()
    h1, ao_d, mean, rstd = ops.xlnet_oproj_ln(cu(av), cu(h), planes, cu(gam), cu(bet), EPS, drop)
    check(f"{tag} ao", ao_d, ao, e_ao, 3e-6)
    check(f"{tag} h1", h1, xh * gam + bet, R.ln_fwd_bound(x, e_x, gam, bet, EPS), 5e-6)
    gg = dy * gam
    dx = rs * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True))
    dao = dx * m
    e_dx = R.ln_bwd_bound(x, e_x, dy, gam, EPS)
    dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    dh, dao_d, dav = ops.xlnet_ln1_bwd(cu(dy), ao_d, cu(h), mean, rstd, cu(gam), planes, dg, db, drop)
    check(f"{tag} dh", dh, dx, e_dx, 2e-5)
    check(f"{tag} dao", dao_d, dao, m * e_dx, 2e-5)
    # the d ao rows carry their own scale, taken from the device's maximum: the floor at half the restated scale
    check(f"{tag} dav", dav, dao @ wo, R.split_bound(dao, wo, row_scale(dao) * 0.5, s_o, ea=m * e_dx), 2e-5)
    check(f"{tag} d_gamma", dg.view(1, -1), (dy * xh).sum(0).view(1, -1), None, 3e-5)
    check(f"{tag} d_beta", db.view(1, -1), dy.sum(0).view(1, -1), None, 3e-5)
    zero_dy = (dy == 0).all(dim=1)
    if bool(zero_dy.any()):
        for t in (dh, dao_d, dav):
            assert float(c64(t)[zero_dy].abs().max()) == 0.0
    if name in ("Etok", "Eweight"):
        assert float(ao_d.abs().max()) == 0.0
    if name == "Eweight":
        assert float(dav.abs().max()) == 0.0
    if name == "Edy":
        assert all(float(t.abs().max()) == 0.0 for t in (dh, dao_d, dav, dg, db))
    check.done()


# ================================================================================================ token-stationary GEMM
@pytest.mark.parametrize("name", ["A0", "A1", "A2", "A4", "B"])      # A3 scales only a gradient: a plain product has none
@pytest.mark.parametrize("M,N,K,tb", [(640, 128, 128, True), (640, 128, 128, False), (600, 96, 64, True), (600, 96, 64, False)])
def test_tok_gemm_every_magnitude_per_row(ops, M, N, K, tb, name):
    """csrc/tok_gemm.hip cuts into three bf16 planes (24 bits, fp32's exponent range): no scales and no floor, so the
    two-piece bound holds a fortiori.  Per row, as _tok_gemm_checks does per tensor: e_new <= max(bound, 3 e_gen)."""
    g = torch.Generator().manual_seed(M + N + K + 5 * len(name) + ord(name[-1]))
    A = torch.randn(M, K, generator=g, dtype=F64)
    W = 0.2 * torch.randn(K, N, generator=g, dtype=F64)
    if name == "B":
        A = A * R.row_exponents(M, g)
    else:
        sx, sw, _ = R.A_GRID[int(name[1])]
        A, W = A * sx, W * sw
    A, W = R.f32(A), R.f32(W)
    ref = A @ W
    Bd = cu(W.t()) if tb else cu(W)
    with ops.tok_gemm_min_rows(512):
        out = c64(ops.gemm(cu(A), Bd, False, tb))
        with ops.precision("fp32"):
            gen = c64(ops.gemm(cu(A), Bd, False, tb))
    bound = R.split_bound(A, W, row_scale(A), R.matrix_scale(W.float())) + R.U * ref.abs()
    e_new, e_gen, b = (out - ref).abs().amax(1), (gen - ref).abs().amax(1), bound.amax(1)
    lim = torch.maximum(b, 3 * e_gen)
    keep = ~R.left_out_rows(ref)
    assert int((~keep).sum()) <= 0.02 * M
    ratio = torch.where(lim > 0, e_new / lim.clamp_min(1e-300), torch.where(e_new > 0, math.inf, 0.0).to(F64))[keep]
    print(f"tok_gemm {name} {M}x{N}x{K} tb={tb}: worst error / limit {float(ratio.max()):.3f}, "
          f"tensor-relative {R.tensor_rel(out, ref):.2e} (general kernel {R.tensor_rel(gen, ref):.2e})")
    assert bool(torch.isfinite(out).all()) and float(ratio.max()) <= 1.0
    assert R.tensor_rel(out, ref) < max(2e-6, 3 * R.tensor_rel(gen, ref))
    if name == "B":
        assert float(out[(A == 0).all(1)].abs().max()) == 0.0


# ================================================================================================ one-kernel attention block
# family A here: the entries of the head's grid with sx sw <= 1.  A2 (5e11, 7e-9) gives scores of 1e7, whose fp32 rounding alone
# is of order 1 before the exponential; A3 scales only an upstream gradient, which a forward does not take.
@pytest.mark.parametrize("with_len", [False, True])
@pytest.mark.parametrize("fam", ["B", "A0", "A1", "A4"])
@pytest.mark.parametrize("B,L,D,n", [(3, 20, 64, 4), (3, 17, 32, 2), (2, 32, 128, 4)])
def test_attn_block_projections_every_magnitude(ops, B, L, D, n, fam, with_len):
    assert ops.xlnet_attn_block_supported(L, D, n)
    g = torch.Generator().manual_seed(100 * B + L + D + ord(fam[-1]))
    T = B * L
    p = dict(R.ff_params(g, D), **other_params(g, D, n, 0.15))
    h = torch.randn(T, D, generator=g, dtype=F64)
    if fam == "B":
        h = h * R.row_exponents(T, g, -6, 6)
    else:
        sx, sw, _ = R.A_GRID[int(fam[1])]
        h = h * sx
        for k in "qkv":
            p[k] = p[k] * sw
    h, p = R.f32(h), {k: R.f32(v) for k, v in p.items()}
    kr = R.f32(0.3 * torch.randn(2 * L, D, generator=g, dtype=F64))
    key_len = torch.randint(1, L + 1, (B,), generator=g) if with_len else None
    planes = ops.xlnet_layer_prepare([cu(p[k]) for k in ORDER], D)
    kl = None if key_len is None else key_len.to(DEV).to(torch.int32)
    h1, saved = ops.xlnet_attn_block_fwd(cu(h), planes, cu(p["o"]).view(D, D), cu(kr).view(-1, D), cu(p["r_w_bias"]).view(-1),
                                          cu(p["r_r_bias"]).view(-1), cu(p["ln_w"]), cu(p["ln_b"]), B, L, n, EPS, 0.0, SEED,
                                          CTR_A, CTR_O, key_len=kl)
    ones = torch.ones(B, n, L, L, dtype=F64)
    ref = attn_reference(p, h, kr, B, L, n, EPS, ones, torch.ones(T, D, dtype=F64), key_len)
    tag, check = f"attn_block {fam} B={B} L={L} D={D} len={with_len}", Checks()
    for z, nm in enumerate("qkv"):
        w = p[nm].reshape(D, D)
        check(f"{tag} {nm}", saved["qkv"][z], ref["qkv"][z],
              R.split_bound(h, w, row_scale(h), R.matrix_scale(w.float())) + R.U * ref["qkv"][z].abs(), 3e-6)
    # behind the softmax (derivation: body_split_restatement, "Behind the softmax"): every row against the propagated bound; the
    # unit-scale 6e-6 of tests/test_attn_block_gpu.py over the rows whose scores fp32 can round to within it (|s| <= 100)
    bd = R.attn_bounds(p, h, kr, B, L, n, ref, key_len, EPS)
    benign = bd["benign"]
    for nm in ("av", "ao", "h1", "mean", "rstd"):
        got = c64(h1 if nm == "h1" else saved[nm]).view(T, -1)
        want = ref[nm].view(T, -1)
        check(f"{tag} {nm}", got, want, bd[nm])
        e = float((got - want)[benign].abs().max() / want.abs().max()) if bool(benign.any()) else 0.0
        assert e < 6e-6, (nm, e)
    e_lse = (c64(saved["lse"]) - ref["lse"]).abs()
    assert bool((e_lse <= bd["lse"]).all()), float((e_lse / bd["lse"]).max())
    ok = (bd["smax"] * R.U <= 6e-6)
    assert float(e_lse[ok].max() if bool(ok.any()) else 0.0) < 6e-6 * max(1.0, float(ref["lse"].abs().max()))
    print(f"{tag}: {int(benign.sum())} of {T} rows with scores within 100, lse worst error / bound {float((e_lse / bd['lse']).max()):.3f}")
    check.done()


# ================================================================================================ whole layer
LAYER_SHAPES = [(6, 20, 64, 4), (9, 20, 128, 4)]
LAYER_AG = [(1.0, 1.0), (2.0 ** 12, 2.0 ** -20), (2.0 ** -12, 2.0 ** 20), (1.0, 2.0 ** -30)]
L0_OUT, L0_GRAD = 1e-5, 3e-5      # tests/test_fused_gpu.py: hout, backward
E32_FACTOR = 4.0


# The weight-gradient GEMMs read the producers' maxima only in the split form, which "auto" takes from 2 GFLOP per product
# (csrc/gemm_f32.hip): these shapes are 100x below that, so the layer tests force it.  With the maxima announced,
# "fp32_bf16x3" runs the two feed-forward weight gradients in the two-way fp16 form (gemm_kernel.h: PREC 4).
SPLIT_MODE = "fp32_bf16x3"


def assert_split_form(grads, grads_fp32):
    """the run under test took the split form: its feed-forward weight gradients are not the fp32 matrix cores' bits"""
    for k in ("w1", "w2"):
        i = ORDER.index(k)
        assert not torch.equal(grads[i], grads_fp32[i]), f"d {k}: the bits of the fp32 form -- the maxima were not read"


def layer_inputs(B, L, D, n, a, gs, seed=0):
    """the magnitudes go through the parameters (the LayerNorms absorb a scaled h): ln_w, ln_b, w2, b2 times a, w1 over a,
    dout times g with the per-row family B on top (80 % of its rows exactly zero)"""
    g = torch.Generator().manual_seed(B + L + D + seed)
    p = dict(R.ff_params(g, D), **other_params(g, D, n))
    for k in ("ln_w", "ln_b", "w2", "b2"):
        p[k] = p[k] * a
    p["w1"] = p["w1"] / a
    p = {k: R.f32(v) for k, v in p.items()}
    h = R.f32(torch.randn(B, L, D, generator=g, dtype=F64))
    dout = torch.randn(B * L, D, generator=g, dtype=F64) * gs * R.row_exponents(B * L, g) * R.mlm_rows(B * L, g)
    return p, h, R.f32(dout).view(B, L, D)


def layer_masks(ops, B, L, D, n, p_drop, seed, offset, layer):
    """the device's keep decisions (0 / 1) per site: the oracle applies 1 / (1 - p) itself"""
    C = lambda site: ops.dropout_ctr_hi(offset, layer, site)
    keep = lambda shape, ctr: (_mask(ops, shape, p_drop, seed, ctr) > 0).double()
    return dict(pos=keep((B, 2 * L, D), ops.dropout_ctr_hi(offset, 255, ops.SITE_POS)), prob=keep((B, n, L, L), C(ops.SITE_PROB)),
                attn_out=keep((B, L, D), C(ops.SITE_ATTN_OUT)), ff_act=keep((B, L, 4 * D), C(ops.SITE_FF_ACT)),
                ff_out=keep((B, L, D), C(ops.SITE_FF_OUT)))


def oracle_layer(p, h, dout, n, dtype, masks, p_drop):
    pr = {k: v.detach().to(dtype).clone().requires_grad_() for k, v in p.items()}
    hr = h.detach().to(dtype).clone().requires_grad_()
    if masks is None:
        out = O.xlnet_layer(hr, pr, n, EPS)
    else:
        out = O.xlnet_layer_dropout(hr, pr, n, EPS, {k: v.to(dtype) for k, v in masks.items()}, p_drop)
    out.backward(dout.to(dtype))
    res = {k: pr[k].grad.double() for k in ORDER}
    res.update(out=out.detach().double(), dh=hr.grad.double())
    return res


@pytest.mark.parametrize("a,gs", LAYER_AG)
@pytest.mark.parametrize("drop_p", [0.0, 0.3])
@pytest.mark.parametrize("B,L,D,n", LAYER_SHAPES)
def test_layer_gradients_every_magnitude(ops, B, L, D, n, drop_p, a, gs):
    """every parameter gradient and d h, tensor-relative, within max(L0, 4 e32): L0 the unit-scale limit, e32 the error of the
    fp32 evaluation of the oracle on the same inputs (4: the split-K summation order of the weight gradients; measured on an
    MI355X the worst error / e32 over the 16 cases is 2.22 -- twice that is not below 4, so the factor stays)"""
    p, h, dout = layer_inputs(B, L, D, n, a, gs)
    seed, offset, layer = 99, 7, 2
    masks = layer_masks(ops, B, L, D, n, drop_p, seed, offset, layer) if drop_p > 0 else None
    ref = oracle_layer(p, h, dout, n, F64, masks, drop_p)
    f32r = oracle_layer(p, h, dout, n, F32, masks, drop_p)
    pos = cu(O.xlnet_pos_emb(L, D))
    params = [cu(p[k]) for k in ORDER]
    kw = dict(drop_p=drop_p, seed=seed, offset=offset, layer_idx=layer)
    h2 = cu(h).view(B * L, D)
    def run(mode):
        with ops.precision(mode):
            out, ws = ops.xlnet_layer_fwd(h2, pos, params, B, L, n, EPS, **kw)
            grads = [torch.zeros_like(t) for t in params]
            dh = ops.xlnet_layer_bwd(h2, pos, params, grads, ws, cu(dout).view(B * L, D), B, L, n, EPS, **kw)
            torch.cuda.synchronize()
        return out, dh, grads
    out, dh, grads = run(SPLIT_MODE)
    assert_split_form(grads, run("fp32")[2])
    worst, worst32 = 0.0, 0.0
    for k, got in [("out", out), ("dh", dh)] + list(zip(ORDER, grads)):
        want = ref[k].reshape(got.shape)
        e32 = R.tensor_rel(f32r[k].reshape(got.shape), want)
        lim = max(L0_OUT if k == "out" else L0_GRAD, E32_FACTOR * e32)
        e = R.tensor_rel(c64(got), want)
        worst, worst32 = max(worst, e / lim), max(worst32, e / e32 if e32 > 0 else 0.0)
        assert bool(torch.isfinite(got).all()) and e <= lim, (k, e, e32, lim)
    print(f"layer B={B} L={L} D={D} p={drop_p} a={a:g} g={gs:g}: worst error / limit {worst:.3f}, worst error / e32 {worst32:.2f}")


def _layer_run(ops, shape, drop_p, a, gs, ws, bws, rows, fuse_final, budget=0, mode=SPLIT_MODE):
    B, L, D, n = shape
    p, h, dout = layer_inputs(B, L, D, n, a, gs, seed=3)
    dout = dout.reshape(B * L, D).clone()
    pos = cu(O.xlnet_pos_emb(L, D))
    params = [cu(p[k]) for k in ORDER]
    kw = dict(drop_p=drop_p, seed=11, offset=3, layer_idx=1 | (ops.LAYER_FUSE_FINAL if fuse_final else 0))
    rk = {}
    if rows is not None:
        keep = torch.zeros(B * L, dtype=torch.bool)
        keep[rows.long().cpu()] = True
        dout[~keep] = 0
        rk = dict(rows=rows, n_rows=int(rows.numel()))
    h2 = cu(h).view(B * L, D)
    grads = [torch.zeros_like(t) for t in params]
    with ops.precision(mode):
        out, _ = ops.xlnet_layer_fwd(h2, pos, params, B, L, n, EPS, ws=ws, **kw, **rk)
        ops.xlnet_set_cu_budget(budget)      # > 0: the backward's token-tile launches plan for that many CUs -- another grid than the forward's
        try:
            dh = ops.xlnet_layer_bwd(h2, pos, params, grads, ws, cu(dout), B, L, n, EPS, bws=bws, **kw, **rk)
            torch.cuda.synchronize()
        finally:
            ops.xlnet_set_cu_budget(0)
    return [out.clone(), dh.clone()] + [t.clone() for t in grads]


@pytest.mark.parametrize("form", ["plain", "rows", "budget"])
@pytest.mark.parametrize("drop_p", [0.0, 0.3])
@pytest.mark.parametrize("shape", LAYER_SHAPES)
def test_layer_workspaces_carry_no_maxima_between_calls(ops, shape, drop_p, form):
    """forward + backward at one magnitude, then at another 2^24 / 2^40 away INTO THE SAME WORKSPACES (both orders), the weight
    gradients in the split form that reads the maxima (SPLIT_MODE; shown by their bits differing from the fp32 form's): the second
    run's bits are those of the same inputs on freshly zeroed workspaces.  'rows': the row-mapped last-layer form with a map
    that leaves a ragged compact tile.  'budget': the backward plans for 4 CUs, so its token-tile launches take 32- / 48-row
    tiles and write 4 maxima slots where the forward's 16-row tiles wrote 8 / 12 -- the weight gradients then also agree with
    the default grid's to rounding (the limit of tests/test_round5_gpu.py's budget test)."""
    B, L, D, n = shape
    rows = None
    if form == "rows":
        gi = torch.Generator().manual_seed(B)
        rows = torch.sort(torch.randperm(B * L, generator=gi)[:37])[0].to(torch.int32).to(DEV)
    fuse = form == "rows" and drop_p > 0
    budget = 4 if form == "budget" else 0
    assert ops.xlnet_get_cu_budget() == 0
    nws = ops.xlnet_layer_ws_floats(B, L, D, n, drop_p > 0)
    nbws = ops.xlnet_layer_bwd_ws_floats(B, L, D, n, drop_p > 0)
    zeros = lambda k: torch.zeros(k, device=DEV, dtype=F32)
    big, small = (2.0 ** 12, 2.0 ** 20), (2.0 ** -12, 2.0 ** -20)
    for first, second in ((big, small), (small, big)):
        fresh = _layer_run(ops, shape, drop_p, *second, zeros(nws), zeros(nbws), rows, fuse, budget)
        ws, bws = zeros(nws), zeros(nbws)
        _layer_run(ops, shape, drop_p, *first, ws, bws, rows, fuse, budget)
        reused = _layer_run(ops, shape, drop_p, *second, ws, bws, rows, fuse, budget)
        for k, x, y in zip(("out", "dh") + tuple(ORDER), fresh, reused):
            assert bool(torch.isfinite(x).all()), k
            assert torch.equal(x, y), f"{k}: max |d| {float((x - y).abs().max()):.3e} after a call at another magnitude"
        assert all(float(t.abs().max()) > 0 for t in fresh)
        assert_split_form(fresh[2:], _layer_run(ops, shape, drop_p, *second, zeros(nws), zeros(nbws), rows, fuse, budget, "fp32")[2:])
        if budget:
            plain = _layer_run(ops, shape, drop_p, *second, zeros(nws), zeros(nbws), rows, fuse)
            for k, x, y in zip(("out", "dh") + tuple(ORDER), fresh, plain):
                assert float((x - y).abs().max()) <= 4e-6 * float(y.abs().max()), k
    print(f"stale maxima {form} B={B} L={L} D={D} p={drop_p}: second run bit-identical to fresh workspaces, both orders")
