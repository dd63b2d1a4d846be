"""The error budget of the body's two-way fp16 split (tests/body_split_restatement.py), checked without a GPU on the input
families of tests/test_body_split_gpu.py at the smallest shape:
  * the restated arithmetic with the project's scale policies stays inside split_bound / the chained FF bounds against fp64;
  * the same arithmetic with one scale per 16-row tile, or one per tensor, for the token operand LEAVES the bound on the
    per-row-magnitude family -- the inputs discriminate (CPU arithmetic only: no kernel is altered for it);
  * everything is finite whenever the fp32 evaluation of the chain is;
  * the fp64 reference alone leaves no more than 2 % of the rows out.
"""
import pytest
import torch

import body_split_restatement as R

T, D = 37, 32
F64, F32 = torch.float64, torch.float32


def _masks(T, D, drop_p, seed):
    if drop_p == 0:
        return torch.ones(T, 4 * D, dtype=F64), torch.ones(T, D, dtype=F64), 1.0
    g = torch.Generator().manual_seed(seed)
    keep = 1.0 - drop_p
    inv_keep = float(torch.tensor(1.0, dtype=F32) / torch.tensor(keep, dtype=F32))
    return ((torch.rand(T, 4 * D, generator=g) < keep).to(F64) * inv_keep, (torch.rand(T, D, generator=g) < keep).to(F64) * inv_keep,
            inv_keep)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in R.FF_FAMILIES:
        h1, p, dy, drop_p = R.ff_family(name, T, D)
        ma, mo, inv_keep = _masks(T, D, drop_p, 5)
        ref = R.ff_chain(R.Exact(F64), h1, p, dy, ma, mo)
        out[name] = dict(h1=h1, p=p, dy=dy, ma=ma, mo=mo, inv_keep=inv_keep, ref=ref,
                         bounds=R.ff_bounds(ref, h1, p, dy, ma, mo, inv_keep))
    return out


def test_pow2_scale_and_cut():
    s = R.pow2_scale(torch.tensor([0.0, float("inf"), float("nan"), 1.0, 0.75, 16383.9, 16384.0, 1e-38, 3.4e38]))
    assert s.tolist() == [1.0, 1.0, 1.0, 2.0 ** 13, 2.0 ** 14, 1.0, 0.5, 2.0 ** 100, 1.0]
    g = torch.Generator().manual_seed(1)
    m = torch.rand(1000, generator=g) * torch.ldexp(torch.ones(1000), torch.randint(-80, 80, (1000,), generator=g))
    top = m * R.pow2_scale(m)
    assert bool(((top >= 2.0 ** 13) & (top < 2.0 ** 14)).all())
    # two pieces: 22 bits down to 2^-3, the absolute floor 2^-25 below
    v = (torch.rand(4000, generator=g, dtype=F32) * 2 - 1) * torch.ldexp(torch.ones(4000), torch.randint(-30, 15, (4000,), generator=g))
    hi, lo = R.cut2(v)
    err = (hi.double() + lo.double() - v.double()).abs()
    assert bool((err <= torch.maximum(v.double().abs() * 2.0 ** -22, torch.tensor(2.0 ** -25, dtype=F64))).all())
    assert bool((lo.double().abs() <= torch.maximum(v.double().abs() * 2.0 ** -11, torch.tensor(2.0 ** -25, dtype=F64))).all())


@pytest.mark.parametrize("K,F", [(32, 32), (128, 96), (512, 32)])
def test_single_product_inside_split_bound(K, F):
    g = torch.Generator().manual_seed(K + F)
    a = R.f32(torch.randn(T, K, generator=g, dtype=F64) * R.row_exponents(T, g))
    a[:, 3] *= 2.0 ** 20                                     # a channel outside the window: the floor term carries the rest
    for sw_ in (1.0, 2e7, 7e-9):
        w = R.f32(torch.randn(K, F, generator=g, dtype=F64) * 0.1 * sw_)
        sa, sw = R.pow2_scale(R.row_amax(a.float())), R.matrix_scale(w.float())
        y = R.split_mm(a.float(), w.float(), sa, sw)
        ratio, left = R.row_ratio(y, a @ w, R.split_bound(a, w, sa, sw))
        print(f"split_mm K={K} F={F} sw={sw_:g}: worst error / bound {ratio:.3f} ({left} rows left out)")
        assert ratio <= 1.0 and bool(torch.isfinite(y).all())


@pytest.mark.parametrize("name", R.FF_FAMILIES)
def test_project_policies_stay_inside_the_bound(cases, name):
    c = cases[name]
    got = R.ff_chain(R.Split(D, c["inv_keep"]), c["h1"], c["p"], c["dy"], c["ma"], c["mo"])
    f32c = R.ff_chain(R.Exact(F32), c["h1"], c["p"], c["dy"], c["ma"], c["mo"])
    for k in R.FF_ROW_OUTPUTS:
        ratio, left = R.row_ratio(got[k], c["ref"][k], c["bounds"][k])
        print(f"restatement {name} T={T} D={D} {k}: worst error / bound {ratio:.3f} ({left} rows left out)")
        assert ratio <= 1.0, (name, k)
        if bool(torch.isfinite(f32c[k]).all()):
            assert bool(torch.isfinite(got[k]).all()), (name, k)
    # the fp32 chain itself sits inside the same budget: the bound is not tighter than the precision it claims
    for k in R.FF_ROW_OUTPUTS:
        assert R.row_ratio(f32c[k], c["ref"][k], c["bounds"][k])[0] <= 1.0, (name, k)


@pytest.mark.parametrize("mode", ["tile", "tensor"])
def test_shared_token_scales_leave_the_bound_on_family_b(cases, mode):
    c = cases["B"]
    got = R.ff_chain(R.Split(D, c["inv_keep"], mode=mode), c["h1"], c["p"], c["dy"], c["ma"], c["mo"])
    for k in ("ffpre", "ffout", "dpre", "dh1"):
        ratio, _ = R.row_ratio(got[k], c["ref"][k], c["bounds"][k])
        print(f"restatement B with one scale per {mode}, {k}: worst error / bound {ratio:.3g}")
        assert ratio > 10.0, (mode, k)
    # while the tensor-relative metric of the unit-scale tests does not see it
    assert R.tensor_rel(got["ffpre"], c["ref"]["ffpre"]) < 3e-6


@pytest.mark.parametrize("name", R.FF_FAMILIES)
@pytest.mark.parametrize("d", [32, 64, 128])
def test_reference_leaves_at_most_two_percent_of_rows_out(name, d):
    h1, p, dy, drop_p = R.ff_family(name, T, d)
    ma, mo, _ = _masks(T, d, drop_p, 5)
    ref = R.ff_chain(R.Exact(F64), h1, p, dy, ma, mo)
    for k in R.FF_ROW_OUTPUTS:
        assert int(R.left_out_rows(ref[k]).sum()) <= 0.02 * T, (name, k)
        assert bool(torch.isfinite(ref[k]).all())
