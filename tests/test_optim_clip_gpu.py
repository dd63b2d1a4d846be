"""Global-norm gradient clipping and AdamW on the device (csrc/optim.hip, include/t4r_hip_optim.h: t4r_grad_sumsq,
t4r_grad_clip_coef, t4r_adamw_step) and their driver optim.FusedAdam(max_grad_norm=..., decoupled_weight_decay=...).

  * the norm: against fl32(|gs| * sqrt(sum double(g)^2)) from float64, to ONE fp32 ulp.  The bound is derived, not measured: the
    device squares and adds in double, a float squared is exact in double, and a double sum of at most 2^31 non-negative terms
    is good to n * 2^-53 relative whatever its order -- far below half an fp32 ulp --, so only the final rounding can differ.
  * the step with no coefficient (or one of exactly 1.0) and coupled decay: the bits of t4r_adam_step / t4r_adam_step_amax.
  * clipped AdamW / Adam steps: against clip_grad_norm_ + torch.optim.AdamW / Adam(foreach=False) in float64 with the
    hyper-parameters rounded to fp32 first, in the units and under the rule of tests/test_adam_gpu.py,
        E_dev <= 2 * E_t32 + 4      after every step, in units of 2^-24 * (|p_ref| + lr),
    E_t32 being torch's fp32 CPU optimizer fed gradients multiplied in fp32 by the coefficient that the fp32 formula gives on
    the float64 norm (torch's own fp32 clip_grad_norm_ is not the yardstick: its norm is tens of ulps off).
  * the table maximum, red zones round every buffer, and the public path on a model."""
import math

import numpy as np
import pytest
import torch

import test_abi_redzone_gpu as rz

pytestmark = pytest.mark.gpu
DEV = "cuda"
WG = 256 * 4                       # elements one workgroup covers per trip (256 threads x float4), all three kernels
SUMSQ_TRIP = WG * 2048             # ... and one trip of the capped grid: t4r_grad_sumsq (2048 workgroups),
PLAIN_TRIP = WG * 4096             # t4r_adamw_step without amax_part (the grid of t4r_adam_step)
AMAX_TRIP = WG * 512               # and with it (the grid of t4r_adam_step_amax)


def sizes(trip):
    return [1, 3, 4, 5, WG - 1, WG, WG + 1, trip + 5, 2 * trip + WG + 3]


# t4r_grad_sumsq reads four trips at a time while four remain: one size that takes that loop, its remainder and the scalar tail
SUMSQ_SIZES = sizes(SUMSQ_TRIP) + [4 * SUMSQ_TRIP + WG + 3]


@pytest.fixture(scope="module")
def ops():
    from transformers4rec_amd import ops as _ops

    return _ops


def f32(x):
    return float(np.float32(x))


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a).cpu(), bits(b).cpu())


def ulps_apart(a, b):
    """distance in fp32 ulps between two positive finite floats"""
    a, b = np.float32(float(a)), np.float32(float(b))
    assert np.isfinite(a) and np.isfinite(b) and a > 0 and b > 0, (a, b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def units(p, p_ref, lr):
    """max over the elements of |p - p_ref| in units of 2^-24 * (|p_ref| + lr)  (tests/test_adam_gpu.py)"""
    p_ref = p_ref.detach().double()
    return float(((p.detach().cpu().double() - p_ref).abs() / (2.0 ** -24 * (p_ref.abs() + lr))).max())


def spread_grad(n, g):
    """gradient magnitudes spread over 1e-4 .. 1e2, every 7th element (from element 2) zero: tests/test_adam_gpu.py's"""
    gr = torch.randn(n, generator=g) * 10.0 ** (6.0 * torch.rand(n, generator=g) - 4.0)
    gr[2::7] = 0.0
    return gr


def ref_norm(grads, gs):
    """fl32(|gs| * sqrt(sum of double(g)^2)) over the buckets"""
    s = sum(float((g.double() ** 2).sum()) for g in grads)
    return np.float32(abs(gs) * math.sqrt(s))


def coef_of(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s arithmetic in fp32 on an fp32 norm"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.minimum(np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6)), np.float32(1.0))


SENTINEL = -7.0


def device_norm(ops, grads, gs, max_norm):
    """the three launches' first two over the buckets -> (out2 on the host, partials on the host, count)"""
    cap = sum(ops.grad_sumsq_parts(g.numel()) for g in grads)
    part = torch.full((cap + 16,), SENTINEL, device=DEV, dtype=torch.float64)
    out = torch.full((2,), SENTINEL, device=DEV)
    n = 0
    for g in grads:
        k = ops.grad_sumsq_(g, part[n:])
        assert k == ops.grad_sumsq_parts(g.numel())
        n += k
    ops.grad_clip_coef_(part, n, gs, max_norm, out)
    pc = part.cpu()
    assert n == cap and bool((pc[n:] == SENTINEL).all()), "a slot beyond the returned count was written"
    assert bool((pc[:n] >= 0).all())
    return out.cpu(), pc, n


# ------------------------------------------------------------------------------------------------------------ 1. the norm
@pytest.mark.parametrize("n", SUMSQ_SIZES)
def test_norm_to_one_ulp(ops, n):
    g = torch.Generator().manual_seed(n % 9973 + 17)
    gr = spread_grad(n, g)
    gd = gr.to(DEV)
    keep = bits(gd).clone()
    for gs, max_norm in ((1.0, 1.0), (0.125, 3.0), (-0.5, 1e4)):
        out, part, cnt = device_norm(ops, [gd], gs, max_norm)
        want = ref_norm([gr], gs)
        d = ulps_apart(out[0], want)
        print(f"norm n={n} gs={gs}: device {float(out[0])!r} float64 {float(want)!r} ({d} ulp), coef {float(out[1])!r}, {cnt} partials")
        assert d <= 1, (n, gs, float(out[0]), float(want))
        # the coefficient is the fp32 formula on the device's OWN norm, bit for bit
        assert same_bits(out[1], torch.tensor(coef_of(out[0].numpy(), max_norm)))
        out2, part2, _ = device_norm(ops, [gd], gs, max_norm)
        assert same_bits(out, out2) and torch.equal(part.view(torch.int64), part2.view(torch.int64))     # run to run
    assert torch.equal(bits(gd), keep)                                                   # the gradient is only read
    out, _, _ = device_norm(ops, [gd], 1.0, float("inf"))
    assert float(out[1]) == 1.0 and ulps_apart(out[0], ref_norm([gr], 1.0)) <= 1


@pytest.mark.parametrize("value,n", [(1e18, 4099), (1e20, 4099), (1e-30, 4099), (1e-30, 3)])
def test_norm_of_very_large_and_very_small_gradients(ops, value, n):
    """one large element among zeros (1e18; 1e20, whose fp32 square is inf) and a buffer of all 1e-30 (every fp32 square is 0):
    squared in double, the norm is finite, non-zero and within 1 ulp"""
    gr = torch.zeros(n)
    if value > 1:
        gr[n - 2] = value                                                                # in the n % 4 tail
    else:
        gr.fill_(value)
    if value != 1e18:                                                                    # what an fp32 sum of squares gives
        assert not bool(torch.isfinite(gr * gr).all()) or float((gr * gr).sum()) == 0.0
    out, _, _ = device_norm(ops, [gr.to(DEV)], 1.0, 1.0)
    want = ref_norm([gr], 1.0)
    assert np.isfinite(want) and want > 0
    assert ulps_apart(out[0], want) <= 1, (float(out[0]), float(want))
    assert same_bits(out[1], torch.tensor(coef_of(out[0].numpy(), 1.0)))
    assert float(out[1]) == (1.0 if value < 1 else f32(np.float32(1.0) / np.float32(out[0])))


def test_norm_of_two_buckets_is_the_norm_of_the_concatenation(ops):
    g = torch.Generator().manual_seed(5)
    a, b = spread_grad(1029, g), spread_grad(70_001, g)
    out, _, cnt = device_norm(ops, [a.to(DEV), b.to(DEV)], 0.25, 1.0)
    assert cnt == 2 + 69
    want = ref_norm([torch.cat([a, b])], 0.25)
    assert ulps_apart(out[0], want) <= 1
    one, _, _ = device_norm(ops, [torch.cat([a, b]).to(DEV)], 0.25, 1.0)
    assert ulps_apart(out[0], one[0]) <= 1 and float(out[1]) < 1.0


# ------------------------------------------------------------------------------- 2. bit identity with the existing entries
def _identity_run(ops, n, amax, wd, gs, coef):
    g = torch.Generator(device=DEV).manual_seed(n % 9973 + int(1000 * wd) + (7 if amax else 0))
    p0 = torch.randn(n, generator=g, device=DEV)
    old = [p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    new = [p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    hp = dict(lr=f32(1e-3), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=f32(wd))
    part_o, part_n = torch.full((1024,), -1.0, device=DEV), torch.full((1024,), -1.0, device=DEV)
    lo, hi = (min(3, n - 1), n) if n > 1 else (0, 1)
    for k in range(5):
        step = k + 1
        gr = torch.randn(n, generator=g, device=DEV) * 10.0 ** (6.0 * torch.rand(n, generator=g, device=DEV) - 4.0)
        gr[2::7] = 0.0
        go, gn = gr.clone(), gr.clone()
        zero = k % 2 == 0                                            # both settings of zero_grad in every run
        if amax:
            part_o.fill_(-1.0), part_n.fill_(-1.0)
            nb_o = ops.adam_step_amax_(old[0], go, old[1], old[2], step, lo, hi, part_o, grad_scale=gs, zero_grad=zero, **hp)
            nb_n = ops.adamw_step_(new[0], gn, new[1], new[2], step, grad_scale=gs, zero_grad=zero, clip_coef=coef,
                                   amax=(lo, hi, part_n), decoupled=False, **hp)
            assert nb_o == nb_n == min(512, max(1, (n // 4 + 255) // 256))
            assert same_bits(part_o, part_n), (n, step)             # the partial maxima, and the untouched slots
        else:
            ops.adam_step_(old[0], go, old[1], old[2], step, grad_scale=gs, zero_grad=zero, **hp)
            nb = ops.adamw_step_(new[0], gn, new[1], new[2], step, grad_scale=gs, zero_grad=zero, clip_coef=coef,
                                 decoupled=False, **hp)
            assert nb == min(4096, max(1, (n // 4 + 255) // 256))
        for a, b, what in zip(old + [go], new + [gn], "pmvg"):
            assert torch.equal(bits(a), bits(b)), (what, n, step, wd, gs)
        assert torch.equal(bits(gn), torch.zeros_like(bits(gn)) if zero else bits(gr))
    assert not torch.equal(bits(new[0]), bits(p0))


@pytest.mark.parametrize("amax", [False, True], ids=["plain", "amax"])
@pytest.mark.parametrize("pos", range(9))
def test_adamw_entry_without_a_clip_is_the_adam_entry_bit_for_bit(ops, amax, pos):
    """clip_coef null or a device 1.0f, decoupled = 0: p, m, v and grad (and the amax partials) of t4r_adamw_step equal those of
    t4r_adam_step / t4r_adam_step_amax over five steps -- coupled weight decay under the new entry, and nothing existing moved"""
    n = sizes(AMAX_TRIP if amax else PLAIN_TRIP)[pos]
    one = torch.ones(1, device=DEV)
    for wd, gs, coef in ((0.0, 1.0, None), (0.01, 0.125, None), (0.01, 1.0, one), (0.0, 0.125, one)):
        _identity_run(ops, n, amax, wd, gs, coef)


# ---------------------------------------------------------------------------------------- 3. clipped steps against float64
class Float64Run:
    """clip_grad_norm_ + torch.optim.AdamW / Adam(foreach=False) over the buckets in float64, and the fp32 yardstick beside it"""

    def __init__(self, p0s, hp, decoupled, max_norm):
        cls = torch.optim.AdamW if decoupled else torch.optim.Adam
        self.max_norm = max_norm
        self.p64 = [p.double().clone().requires_grad_() for p in p0s]
        self.p32 = [p.float().clone().requires_grad_() for p in p0s]
        self.o64, self.o32 = cls(self.p64, foreach=False, **hp), cls(self.p32, foreach=False, **hp)

    def step(self, grads, lr=None):
        """grads: the scaled fp32 gradients the device sees.  -> (float64-derived fp32 norm, its fp32 coefficient)"""
        if lr is not None:
            for o in (self.o64, self.o32):
                o.param_groups[0]["lr"] = lr
        for p, g in zip(self.p64, grads):
            p.grad = g.double().clone()
        torch.nn.utils.clip_grad_norm_(self.p64, self.max_norm)
        self.o64.step()
        norm = ref_norm(grads, 1.0)
        coef = coef_of(norm, self.max_norm)
        for p, g in zip(self.p32, grads):
            p.grad = g.float() * torch.tensor(coef)                  # one fp32 rounding per element, as the device's
        self.o32.step()
        return norm, coef

    def errors(self, dev_ps, lr):
        e_dev = max(units(d, r, lr) for d, r in zip(dev_ps, self.p64))
        e_t32 = max(units(t, r, lr) for t, r in zip(self.p32, self.p64))
        return e_dev, e_t32


# name -> (p scale, hyper-parameters, decoupled, grad_scale)
CLIP_CASES = {
    "adamw_wd0.01": (0.1, dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01), True, 1.0),
    "adamw_wd0.1_gradscale": (1.0, dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1), True, 0.125),
    "adam_wd0_clip": (1e-3, dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0), False, 1.0),
}
BUCKETS = (1029, 70_001)


@pytest.mark.parametrize("case", list(CLIP_CASES))
def test_clipped_steps_against_fp64(ops, case):
    """two buckets, six steps, max_norm 1; the gradients of steps 2 and 5 are 2^-20 times smaller, so that the clip is inactive
    there (coefficient exactly 1.0) and active on the others.
    Measured on the MI355X, per step (E_dev / E_t32), bound 2 * E_t32 + 4:
      adamw_wd0.01           2.8 / 3.1   5.3 / 5.8   6.2 / 5.1   8.5 / 7.4   13.8 / 9.5   14.4 / 11.0
      adamw_wd0.1_gradscale  2.2 / 3.4   4.0 / 4.0   5.7 / 5.0   6.8 / 6.1    7.1 / 7.1    9.8 / 8.3
      adam_wd0_clip          2.3 / 2.4   4.2 / 5.6   4.2 / 5.7   5.6 / 6.4    7.8 / 8.4    8.5 / 9.1
    coefficient 2.1e-4 ... 2.2e-4 on the active steps, exactly 1.0 on steps 2 and 5.  The smallest margin to the bound is 9.2 units (first case, step 5)."""
    scale, hp, decoupled, gs = CLIP_CASES[case]
    hp = dict(lr=f32(hp["lr"]), betas=(f32(hp["betas"][0]), f32(hp["betas"][1])), eps=f32(hp["eps"]),
              weight_decay=f32(hp["weight_decay"]))
    g = torch.Generator().manual_seed(600 + len(case))
    p0s = [scale * torch.randn(n, generator=g) for n in BUCKETS]
    ref = Float64Run(p0s, hp, decoupled, 1.0)
    dev = [[p.to(DEV).clone(), torch.zeros(p.numel(), device=DEV), torch.zeros(p.numel(), device=DEV)] for p in p0s]
    part = torch.zeros(sum(ops.grad_sumsq_parts(n) for n in BUCKETS), device=DEV, dtype=torch.float64)
    out = torch.zeros(2, device=DEV)
    rows = []
    for step in range(1, 7):
        grads = [spread_grad(n, g) for n in BUCKETS]
        if step in (2, 5):
            grads = [gr * 2.0 ** -20 for gr in grads]
        norm, coef = ref.step(grads)
        gds = [(gr / gs).to(DEV) for gr in grads]                    # grad_scale is a power of two: the product is exact
        n_part = 0
        for gd in gds:
            n_part += ops.grad_sumsq_(gd, part[n_part:])
        ops.grad_clip_coef_(part, n_part, gs, 1.0, out)
        for (p, m, v), gd in zip(dev, gds):
            ops.adamw_step_(p, gd, m, v, step, grad_scale=gs, zero_grad=True, clip_coef=out[1:], decoupled=decoupled, **hp)
            assert not bool(gd.any())
        o = out.cpu()
        assert ulps_apart(o[0], norm) <= 1
        assert (float(o[1]) == 1.0 and float(coef) == 1.0) if step in (2, 5) else (float(o[1]) < 0.01 and float(coef) < 0.01)
        e_dev, e_t32 = ref.errors([d[0] for d in dev], hp["lr"])
        print(f"clip {case} step={step}: coef={float(o[1]):.3e} E_dev={e_dev:.2f} E_t32={e_t32:.2f}")
        rows.append((step, e_dev, e_t32))
    for step, e_dev, e_t32 in rows:
        assert e_dev <= 2.0 * e_t32 + 4.0, (case, step, e_dev, e_t32)


# ------------------------------------------------------------------------------------------ 4. the amax through the new entry
# (n, lo, hi, position of the largest element after the update) -- lo and hi are no multiples of 4
PLANTS = [
    (4099, 1030, 3001, 1030),                      # at lo
    (4099, 1030, 3001, 3000),                      # at hi - 1
    (4099, 5, 4099, 4097),                         # in the n % 4 tail
    (4099, 4097, 4099, 4098),                      # the range lies in the tail, the largest at hi - 1 = n - 1
    (3, 1, 3, 1),                                  # a buffer that is all tail
    (AMAX_TRIP + 1027, 1001, AMAX_TRIP + 1026, AMAX_TRIP + 514),      # second grid-stride trip, float4 body
    (AMAX_TRIP + 1027, AMAX_TRIP + 1, AMAX_TRIP + 1027, AMAX_TRIP + 1),   # range wholly in the second trip, largest at lo
]


@pytest.mark.parametrize("n,lo,hi,at", PLANTS)
def test_adamw_amax_planted_maximum(ops, n, lo, hi, at):
    """max(part[:returned]) == max |p[lo:hi]| after a clipped, decoupled update, bit for bit, with the largest element of the
    range planted at `at` and LARGER elements planted at lo - 1 and at hi (as tests/test_adam_gpu.py does for the old entry)"""
    g = torch.Generator().manual_seed(n + 31 * lo + at)
    p0 = torch.randn(n, generator=g).clamp_(-4.0, 4.0)
    p0[at] = -40.0
    if lo > 0:
        p0[lo - 1] = 100.0
    if hi < n:
        p0[hi] = -100.0
    gr = torch.randn(n, generator=g)
    p, gd, m, v = p0.clone().to(DEV), gr.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    part = torch.full((1024,), -1.0, device=DEV)
    coef = torch.tensor([0.25], device=DEV)
    nb = ops.adamw_step_(p, gd, m, v, 1, lr=1e-2, weight_decay=0.1, decoupled=True, clip_coef=coef, amax=(lo, hi, part))
    assert nb == min(512, max(1, (n // 4 + 255) // 256))
    pc, pt = p.cpu(), part.cpu()
    assert int(pc[lo:hi].abs().argmax()) == at - lo and float(pc[at]) != -40.0       # the planted element, moved by the step
    assert bool((pt[:nb] >= 0).all()) and bool((pt[nb:] == -1.0).all())
    assert same_bits(pt[:nb].max(), pc[at].abs()) and same_bits(pt[:nb].max(), pc[lo:hi].abs().max())
    assert int(pt[:nb].argmax()) == (at % (nb * WG)) // WG


# ------------------------------------------------------------------------------------------------ 5. red zones and poison
def _adamw_ref(p, g, m, v, step, lr, b1, b2, eps, wd, gs, coef, decoupled):
    p, g, m, v = (t.double() for t in (p, g, m, v))
    g = g * gs * coef
    if decoupled:
        p = p * (1 - lr * wd)
    else:
        g = g + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - lr * (m / (1 - b1 ** step)) / ((v / (1 - b2 ** step)).sqrt() + eps)
    return p, m, v


def _rz_chain(n, clip, decoupled, amax):
    """the launches of one bucket's step inside the arena: guards round the gradient, the partials at their exact count, the
    two output floats, the four step buffers and the partial maxima at their exact count"""
    def fn(a, key):
        lib = rz._lib().load()
        g = rz.gen(n + 3)
        p0, gr, m0, v0 = rz.rn(g, n), rz.rn(g, n, scale=3.0), 0.1 * rz.rn(g, n), 0.01 * rz.rn(g, n).abs()
        step, lr, b1, b2, eps, wd, gs, max_norm = 3, 1e-2, 0.9, 0.999, 1e-8, 0.01, 0.5, 0.75
        P, Gd = a.new("param", "inout", rz.F32, n).set(p0), a.new("grad", "inout", rz.F32, n).set(gr)
        M, V = a.new("exp_avg", "inout", rz.F32, n).set(m0), a.new("exp_avg_sq", "inout", rz.F32, n).set(v0)
        outs, coef, coef_ptr = [], 1.0, None
        if clip:
            cnt = lib.t4r_grad_sumsq_parts(n)
            PART = a.new("part", "out", torch.float64, cnt)
            OUT = a.new("out2", "out", rz.F32, 2)
            assert rz.rc_call(a, "t4r_grad_sumsq", rz.stream(), Gd.ptr, n, PART.ptr) == cnt
            rz.call(a, "t4r_grad_clip_coef", rz.stream(), PART.ptr, cnt, gs, max_norm, OUT.ptr)
            norm = rz.memo((key, "norm"), lambda: torch.tensor([float(ref_norm([gr], gs))]))
            coef = float(coef_of(norm.numpy()[0], max_norm))
            coef_ptr = OUT.ptr + 4
            t = "the float64 norm to 1 ulp (test_norm_to_one_ulp), the coefficient from it: 4 ulps of room"
            outs += [rz.Out(OUT, torch.tensor([float(norm), coef]), dict(rtol=5e-7, atol=0.0), t),
                     rz.Out(PART, (gr.double() ** 2).sum().view(1), dict(rtol=1e-12, atol=0.0), "sum of the partials in double (n * 2^-53)",
                            sel=lambda v: v.sum().view(1))]
            outs[-1].atomic = False
        rp, rm, rv = rz.memo((key, "adamw"), lambda: _adamw_ref(p0, gr, m0, v0, step, lr, b1, b2, eps, wd, gs, coef, decoupled))
        t = "test_kernels_gpu.py::test_adam_matches_torch"
        tol = dict(rtol=1e-5, atol=1e-6)
        outs += [rz.Out(P, rp, tol, t), rz.Out(M, rm, tol, t), rz.Out(V, rv, tol, t),
                 rz.Out(Gd, torch.zeros(n), None, "zero_grad clears grad")]
        args = (rz.stream(), P.ptr, Gd.ptr, M.ptr, V.ptr, n, step, lr, b1, b2, eps, wd, int(decoupled), gs, 1, coef_ptr)
        if not amax:
            nb = rz.rc_call(a, "t4r_adamw_step", *args, 0, 0, None)
            assert nb == min(4096, max(1, (n // 4 + 255) // 256))
            return outs
        lo, hi = min(3, n - 1), n
        want = min(512, max(1, (n // 4 + 255) // 256))
        AM = a.new("amax_part", "out", rz.F32, want)
        nb = rz.rc_call(a, "t4r_adamw_step", *args, lo, hi, AM.ptr)
        assert nb == want
        torch.cuda.synchronize()
        amax_ref = P.win[lo:hi].abs().max().cpu().view(1)
        outs.append(rz.Out(AM, amax_ref, None, "max |param| over [lo, hi) of the stored update: exact", sel=lambda v: v.max().view(1)))
        outs[-1].atomic = False
        return outs
    return fn


_CLIP = ["t4r_grad_sumsq", "t4r_grad_clip_coef", "t4r_adamw_step"]
REDZONE_CASES = (
    [rz.Case("optim", f"clip_adamw_amax-{n}", _CLIP, _rz_chain(n, True, True, True)) for n in (1, 3, 4, 5, 1023, 1024, 1025, 4099)]
    + [rz.Case("optim", f"clip_adam-{n}", _CLIP, _rz_chain(n, True, False, False)) for n in (5, 1025)]
    + [rz.Case("optim", f"adamw_noclip-{n}", ["t4r_adamw_step"], _rz_chain(n, False, True, False)) for n in (3, 1023)]
    + [rz.Case("optim", "adam_noclip_amax-1025", ["t4r_adamw_step"], _rz_chain(1025, False, False, True))]
)
_RZ_BY_ID = {c.id: c for c in REDZONE_CASES}


@pytest.mark.parametrize("cid", list(_RZ_BY_ID))
def test_redzone(cid):
    """the three runs of tests/test_abi_redzone_gpu.py::test_redzone over the launching entries of the fourth header: guards round
    every buffer, exact partial counts, both fill bytes, a sibling case in between and a rerun.  No float atomics anywhere:
    every output is bit-identical between the runs."""
    c = _RZ_BY_ID[cid]
    a0, outs0 = rz._run(c, 0x00)
    v0 = rz._values(outs0)
    for o, got in zip(outs0, v0):
        assert bool(torch.isfinite(got).all()), f"{cid}: non-finite value in '{o.buf.name}' under fill 0x00"
        rz._against(o, got, o.ref, f"{cid} fill 0x00")
    del a0
    a1, outs1 = rz._run(c, 0xFF)
    for o, got, first in zip(outs1, rz._values(outs1), v0):
        assert bool(torch.isfinite(got).all()), f"{cid}: non-finite value in '{o.buf.name}' under fill 0xFF"
        assert rz._bits_equal(got, first), f"{cid}: '{o.buf.name}' differs between fill 0x00 and fill 0xFF"
    del a1
    sib = REDZONE_CASES[(REDZONE_CASES.index(c) + 1) % len(REDZONE_CASES)]
    rz._run(sib, 0x00)
    a2, outs2 = rz._run(c, 0x00)
    for o, got, first in zip(outs2, rz._values(outs2), v0):
        assert rz._bits_equal(got, first), f"{cid}: '{o.buf.name}' changed after running {sib.id} in between"


# ------------------------------------------------------------------------------------------------------ 6. the public path
def _small_model():
    """the smallest XLNet MLM model of tests/test_e2e_gpu.py, with the reference's parameters, on the device"""
    import test_e2e_gpu as e2e

    d, model, x, cap, hooks = e2e.run_train_case("xlnet_mlm_item_train", emb_default=32)
    for h in hooks:
        h.remove()
    return model, x


def test_fused_adam_clipped_adamw_on_a_model(ops):
    """three training steps of FusedAdam(weight_decay=0.01, decoupled_weight_decay=True, max_grad_norm=0.05) under a linear
    warm-up against float64 AdamW + clip_grad_norm_ fed the SAME gradients (copied before each step) and the scheduled rate.
    Measured on the MI355X, per step (E_dev / E_t32): 0.0 / 0.0 (the warm-up's first step runs at lr 0), 2.7 / 2.8, 3.5 / 4.4;
    norm 1.9 - 2.2, coefficient 0.022 - 0.027."""
    import transformers4rec_amd as tr

    model, x = _small_model()
    flats = [f for f in tr.flatten_model(model) if f is not None]
    assert len(flats) == 2
    base_lr, wd, max_norm = f32(1e-3), f32(0.01), 0.05
    sched = tr.warmup_schedule("linear", 2, 6)
    opt = tr.FusedAdam(flats, lr=base_lr, weight_decay=wd, decoupled_weight_decay=True, max_grad_norm=max_norm).set_schedule(sched)
    assert opt.last_grad_norm is None
    hp = dict(lr=base_lr, betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=wd)
    ref = Float64Run([f.data.cpu() for f in flats], hp, True, max_norm)
    table = model.input_features.item_embedding_table.weight
    rows = []
    for t in range(1, 4):
        out = model(x, training=True)
        out["loss"].backward()
        grads = [f.grad.cpu().clone() for f in flats]
        assert all(bool(gr.any()) for gr in grads)
        lr_t = f32(base_lr * sched(t - 1))
        norm, coef = ref.step(grads, lr=lr_t)
        opt.step()
        assert opt.step_count == t and f32(opt.lr) == lr_t
        got = opt.last_grad_norm
        assert got.ndim == 0 and got.is_cuda and ulps_apart(got.cpu(), norm) <= 1
        assert float(coef) < 1.0, "the clip must be active for this test to mean anything"
        for f in flats:
            assert not bool(f.grad.any())
        am = ops.w_amax_of(table)
        assert am is not None and same_bits(am[0][:am[1]].max(), table.detach().abs().max())
        e_dev, e_t32 = ref.errors([f.data for f in flats], lr_t if lr_t > 0 else base_lr)      # step 1 runs at lr 0
        print(f"model step={t}: lr={lr_t:.3e} norm={float(norm):.4e} coef={float(coef):.3e} E_dev={e_dev:.2f} E_t32={e_t32:.2f}")
        rows.append((t, e_dev, e_t32))
    assert [f32(base_lr * sched(t)) for t in range(3)] == [0.0, f32(base_lr * 0.5), base_lr]
    for t, e_dev, e_t32 in rows:
        assert e_dev <= 2.0 * e_t32 + 4.0, (t, e_dev, e_t32)


def test_fused_adam_default_arguments_run_the_old_entries(ops):
    """FusedAdam() with its old arguments: the parameters after two steps are, bit for bit, what ops.adam_step_ (dense bucket) and
    ops.adam_step_amax_ (table bucket) leave on clones fed the same gradients -- the path every earlier version ran"""
    import transformers4rec_amd as tr

    model, x = _small_model()
    flats = [f for f in tr.flatten_model(model) if f is not None]
    opt = tr.FusedAdam(flats, lr=2e-3, weight_decay=0.01)
    clones = [[f.data.clone(), torch.zeros_like(f.data), torch.zeros_like(f.data)] for f in flats]
    part = torch.zeros(1024, device=DEV)
    for t in range(1, 3):
        out = model(x, training=True)
        out["loss"].backward()
        grads = [f.grad.clone() for f in flats]
        opt.step(grad_scale=0.5)
        for k, ((p, m, v), gr) in enumerate(zip(clones, grads)):
            tgt = opt._amax_targets[k]
            if tgt is None:
                ops.adam_step_(p, gr, m, v, t, 2e-3, (0.9, 0.999), 1e-8, 0.01, 0.5, zero_grad=True)
            else:
                ops.adam_step_amax_(p, gr, m, v, t, tgt[1], tgt[1] + tgt[0].numel(), part, 2e-3, (0.9, 0.999), 1e-8, 0.01, 0.5,
                                    zero_grad=True)
        assert [tg is None for tg in opt._amax_targets] == [True, False]
        for f, (p, m, v), (om, ov) in zip(flats, clones, opt.state):
            assert torch.equal(bits(f.data), bits(p)) and torch.equal(bits(om), bits(m)) and torch.equal(bits(ov), bits(v)), t
        assert opt.last_grad_norm is None and opt.lr == 2e-3
