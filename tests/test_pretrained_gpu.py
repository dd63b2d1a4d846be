"""The fused gather + projection of pretrained-embedding features (csrc/pretrained_proj.hip, include/t4r_hip_pretrained.h) on the
GPU: both directions against float64 (tests/pretrained_restatement.py) at 4 x the error of torch's own fp32 CPU arithmetic on the
same inputs, bit-exactness, the id clamp, red zones around every buffer, and the module path against the reference's fixture
(tests/golden/xlnet_mlm_pretrained_train.npz, tools/make_pretrained_golden.py).

Figures on one box (kernel error / torch fp32 error, both relative to the largest |output|; `-s` prints them): forward 0.52 to
1.71, median 1.0; gradients 0.17 to 2.31."""

import pytest
import torch

import golden_utils as gu
import pretrained_restatement as R
import transformers4rec_amd as tr
from abi_arena import FILLS, Arena
from transformers4rec_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
V = 37
SHAPES = [(16, 32), (40, 24), (272, 64), (768, 64), (1024, 256), (33, 1)]
F32, F16, I64, I32 = torch.float32, torch.float16, torch.int64, torch.int32


def _case(E, P, seed=0):
    """(table, image on the device, W, b, gamma, beta) -- W, b as torch.nn.Linear draws them"""
    g = torch.Generator().manual_seed(seed * 1000 + E * 7 + P)
    table = torch.randn((V, E), generator=g)
    bound = 1.0 / E ** 0.5
    W = (torch.rand((P, E), generator=g) * 2 - 1) * bound
    b = (torch.rand((P,), generator=g) * 2 - 1) * bound
    gamma = 1 + 0.1 * torch.randn((P,), generator=g)
    beta = 0.1 * torch.randn((P,), generator=g)
    image = ops.pack_item_table(table.to(DEV), "fp16")
    return table, image, W, b, gamma, beta


def _ids(n, seed):
    """ids with pads (row 0), repeats and the last row"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (n,), generator=g)
    ids[0] = V - 1
    if n > 2:
        ids[1] = 0
        ids[n - 1] = ids[n // 2]
    if n > 8:
        ids[3:6] = 0
    return ids


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


@pytest.fixture(scope="module")
def cases():
    return {s: _case(*s) for s in SHAPES}


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("ln", [False, True], ids=["plain", "layernorm"])
@pytest.mark.parametrize("E,P", SHAPES)
def test_forward_against_float64(cases, E, P, ln):
    table, image, W, b, gamma, beta = cases[(E, P)]
    gm, bt = (gamma, beta) if ln else (None, None)
    Wd, bd, gd, btd = _dev(W, b, gm, bt)
    img_cpu = image.cpu()
    worst = 0.0
    runs = [(T, T, 0, 0) for T in (1, 63, 129, 300)] + [(300, 30, 3, 5), (130, 10, 0, 0)]     # (T, number of ids, col, pad after)
    for T, n_ids, col, pad in runs:
        ids = _ids(n_ids, T + n_ids)
        ref = R.forward(img_cpu, ids, T, W, b, gm, bt)
        t32 = R.forward(img_cpu, ids, T, W, b, gm, bt, dtype=torch.float32)
        wide = torch.full((T, col + P + pad), 7.5, device=DEV)
        out, xhat, rstd = ops.pretrained_proj_fwd(image, ids.to(DEV), Wd, bd, gd, btd, T=T, out=wide, col=col)
        got = wide[:, col:col + P].cpu()
        assert bool((wide[:, :col] == 7.5).all()) and bool((wide[:, col + P:] == 7.5).all())
        e_k, e_t = R.rel_err(got, ref), R.rel_err(t32, ref)
        print(f"forward E={E} P={P} ln={ln} T={T} ids={n_ids} col={col}: kernel {e_k:.3e} torch32 {e_t:.3e} ratio "
              f"{e_k / e_t if e_t else float('nan'):.2f}")
        assert e_k <= 4 * e_t, (T, n_ids, col, e_k, e_t)
        worst = max(worst, e_k)
        if ln:
            assert xhat.shape == (T, P) and rstd.shape == (T,) and bool(torch.isfinite(xhat).all())
        else:
            assert xhat is None and rstd is None
    assert worst < 1e-5


def test_a_dropped_lo_plane_would_be_caught(cases):
    """the margin of the bound: W rounded to its hi plane alone misses it by two orders of magnitude"""
    table, image, W, b, _g, _b = cases[(768, 64)]
    ids = _ids(300, 5)
    ref = R.forward(image.cpu(), ids, 300, W, b)
    e_t = R.rel_err(R.forward(image.cpu(), ids, 300, W, b, dtype=torch.float32), ref)
    e_hi = R.rel_err(R.forward(image.cpu(), ids, 300, W.half().float(), b, dtype=torch.float32), ref)
    assert e_hi > 100 * e_t


# ------------------------------------------------------------------------------------------------ backward
def _backward(image, ids, T, W, gamma, dY_wide, col, xhat, rstd, acc=None):
    P, E = W.shape
    outs = acc or dict(dW=torch.zeros((P, E), device=DEV), db=torch.zeros(P, device=DEV), dgamma=torch.zeros(P, device=DEV),
                       dbeta=torch.zeros(P, device=DEV))
    ln = gamma is not None
    ops.pretrained_proj_bwd(dY_wide, image, ids, gamma, xhat, rstd, outs["dW"], outs["db"], outs["dgamma"] if ln else None,
                            outs["dbeta"] if ln else None, col=col)
    return outs


@pytest.mark.parametrize("E,P,ln", [(40, 24, True), (40, 24, False), (272, 64, True), (33, 1, True), (33, 1, False), (1024, 256, True),
                                    (768, 64, True)])
def test_backward_against_float64(cases, E, P, ln):
    table, image, W, b, gamma, beta = cases[(E, P)]
    gm, bt = (gamma, beta) if ln else (None, None)
    Wd, bd, gd, btd = _dev(W, b, gm, bt)
    img_cpu = image.cpu()
    for T, n_ids, col in ((1, 1, 0), (300, 300, 0), (2000, 2000, 2), (300, 30, 0)):
        ids = _ids(n_ids, 3 * T + n_ids)
        g = torch.Generator().manual_seed(T)
        dY = torch.randn((T, P), generator=g)
        ref = R.gradients(img_cpu, ids, T, W, b, gm, bt, dY)
        t32 = R.gradients(img_cpu, ids, T, W, b, gm, bt, dY, dtype=torch.float32)
        wide = torch.full((T, col + P + 3), 3.25, device=DEV)
        wide[:, col:col + P] = dY.to(DEV)
        _o, xhat, rstd = ops.pretrained_proj_fwd(image, ids.to(DEV), Wd, bd, gd, btd, T=T)
        got = _backward(image, ids.to(DEV), T, Wd, gd, wide, col, xhat, rstd)
        torch.cuda.synchronize()
        for k, r in ref.items():
            if P == 1 and ln and k in ("dW", "db", "dgamma"):
                # A LayerNorm over ONE output is constant: its xhat is zero and so is the true gradient in front of it (float64
                # autograd returns its own rounding noise, 1e-12), so there is no relative error to take.  The kernel forms rstd * (g - mean(g)) with g = dY * gamma:
                # at worst one fp32 rounding of g per token (a contracted multiply-subtract sees the unrounded product), times
                # rstd = 1 / sqrt(eps), times |x| for d W, summed over the T tokens.
                scale = float(dY.abs().max() * gamma.abs().max()) * (1e-5 ** -0.5) * (float(img_cpu.float().abs().max()) if k == "dW" else 1.0)
                assert float(r.abs().max()) < 1e-9 and float(got[k].abs().max()) <= 2.0 ** -24 * scale * T, (T, k)
                continue
            e_k, e_t = R.rel_err(got[k].cpu(), r), R.rel_err(t32[k], r)
            print(f"backward E={E} P={P} ln={ln} T={T} ids={n_ids} {k}: kernel {e_k:.3e} torch32 {e_t:.3e} ratio "
                  f"{e_k / e_t if e_t else float('nan'):.2f}")
            assert e_k <= 4 * e_t, (T, n_ids, k, e_k, e_t)


# ------------------------------------------------------------------------------------------------ bit-exactness
@pytest.mark.parametrize("E,P", [(40, 24), (768, 64), (1024, 256)])
def test_a_rows_bits_depend_on_its_id_only(cases, E, P):
    table, image, W, b, gamma, beta = cases[(E, P)]
    Wd, bd, gd, btd = _dev(W, b, gamma, beta)
    ids = _ids(300, 9).to(DEV)
    out, xhat, rstd = ops.pretrained_proj_fwd(image, ids, Wd, bd, gd, btd)
    perm = torch.randperm(300, generator=torch.Generator().manual_seed(1)).to(DEV)
    out_p, xhat_p, rstd_p = ops.pretrained_proj_fwd(image, ids[perm], Wd, bd, gd, btd)
    assert torch.equal(out_p, out[perm]) and torch.equal(xhat_p, xhat[perm]) and torch.equal(rstd_p, rstd[perm])
    # another T and launch shape: the same id gives the same row
    out_s, _x, _r = ops.pretrained_proj_fwd(image, ids[7:48].contiguous(), Wd, bd, gd, btd)
    assert torch.equal(out_s, out[7:48])
    same = (ids == ids[150]).nonzero().flatten()
    assert same.numel() > 1 and all(torch.equal(out[i], out[150]) for i in same)


def test_gradients_are_bit_reproducible_and_accumulated(cases):
    table, image, W, b, gamma, beta = cases[(272, 64)]
    Wd, bd, gd, btd = _dev(W, b, gamma, beta)
    T = 2000
    ids = _ids(T, 4).to(DEV)
    dY = torch.randn((T, 64), generator=torch.Generator().manual_seed(2)).to(DEV)
    _o, xhat, rstd = ops.pretrained_proj_fwd(image, ids, Wd, bd, gd, btd)
    a = _backward(image, ids, T, Wd, gd, dY, 0, xhat, rstd)
    c = _backward(image, ids, T, Wd, gd, dY, 0, xhat, rstd)
    for k in a:
        assert torch.equal(a[k], c[k]), k
    twice = _backward(image, ids, T, Wd, gd, dY, 0, xhat, rstd, acc={k: v.clone() for k, v in a.items()})
    for k in a:
        assert torch.equal(twice[k], 2 * a[k]), k       # x + x is exact: the outputs are accumulated, the sum is formed first


# ------------------------------------------------------------------------------------------------ ids out of range
def test_out_of_range_ids_set_the_flag_and_read_a_legal_row(cases):
    table, image, W, b, gamma, beta = cases[(40, 24)]
    Wd, bd, gd, btd = _dev(W, b, gamma, beta)
    ids = _ids(64, 1)
    bad = ids.clone()
    bad[5], bad[40] = V, -1
    err = torch.zeros(1, dtype=I32, device=DEV)
    good, _x, _r = ops.pretrained_proj_fwd(image, ids.to(DEV), Wd, bd, gd, btd, err_flag=err)
    assert int(err.item()) == 0
    out, xhat, rstd = ops.pretrained_proj_fwd(image, bad.to(DEV), Wd, bd, gd, btd, err_flag=err)
    torch.cuda.synchronize()
    assert int(err.item()) == 1
    keep = torch.ones(64, dtype=torch.bool)
    keep[5] = keep[40] = False
    assert torch.equal(out[keep.to(DEV)], good[keep.to(DEV)])
    row0, _x, _r = ops.pretrained_proj_fwd(image, torch.zeros(1, dtype=I64, device=DEV), Wd, bd, gd, btd)
    assert torch.equal(out[5], row0[0]) and torch.equal(out[40], row0[0])
    got = _backward(image, bad.to(DEV), 64, Wd, gd, torch.ones((64, 24), device=DEV), 0, xhat, rstd)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in got.values())


def test_module_check_ids_raises_for_an_attached_table():
    f, x, _table = _sum_block()
    f.pretrained_module.attach_table("vec", _table)
    x = dict(x)
    del x["vec"]
    f(x)
    f.check_ids()
    # the table has fewer rows than the item vocabulary: the last item id is outside it
    f.pretrained_module.attach_table("vec", _table[:-1].contiguous())
    x["item_id"] = x["item_id"].clone()
    x["item_id"][0, 0] = _table.shape[0] - 1
    f(x)
    with pytest.raises(IndexError):
        f.check_ids()


# ------------------------------------------------------------------------------------------------ red zones
def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("fill", FILLS, ids=["zeros", "ones"])
@pytest.mark.parametrize("E,P,T,n_ids", [(40, 24, 129, 129), (33, 1, 63, 63), (272, 64, 300, 30), (1024, 256, 65, 65)])
def test_red_zones_around_every_buffer(cases, fill, E, P, T, n_ids):
    lib = _lib.load()
    table, image, W, b, gamma, beta = cases[(E, P)]
    ldp = image.stride(0)
    col, pad = 5, 3
    a = Arena(fill, DEV, capacity=16 << 20)
    full = torch.as_strided(image, (V, ldp), (ldp, 1))
    img = a.new("image", "in", F16, (V, ldp)).set(full)
    ids = a.new("ids", "in", I64, n_ids).set(_ids(n_ids, 7))
    Wb = a.new("W", "in", F32, P * E).set(W)
    bb = a.new("b", "in", F32, P).set(b)
    gb = a.new("gamma", "in", F32, P).set(gamma)
    btb = a.new("beta", "in", F32, P).set(beta)
    out = a.new("out", "out", F32, (T, col + P + pad), col=col, width=P)
    xh = a.new("xhat", "out", F32, T * P)
    rs = a.new("rstd", "out", F32, T)
    ws = a.ws("ws", lib.t4r_pretrained_proj_ws_bytes(E, P))
    err = a.new("err", "inout", I32, 1).set(0)
    a.seal()
    before = img.bits()
    rc = lib.t4r_pretrained_proj_fwd(_stream(), 3, img.ptr, ldp, V, ids.ptr, T, T // n_ids, Wb.ptr, bb.ptr, gb.ptr, btb.ptr, 1e-5,
                                     E, P, out.ptr, col + P + pad, col, xh.ptr, rs.ptr, ws.ptr, err.ptr)
    assert rc == 0, lib.t4r_last_error()
    torch.cuda.synchronize()
    v = a.check()
    assert v is None, str(v)
    assert a.nonfinite() is None and torch.equal(img.bits(), before) and int(err.t.item()) == 0
    want, _x, _r = ops.pretrained_proj_fwd(image, ids.t, *_dev(W, b, gamma, beta), T=T)
    assert torch.equal(out.win, want)
    # ---- backward, the forward's xhat / rstd now inputs
    ld = col + P + pad
    dY = a.new("dY", "in", F32, (T, ld), col=col, width=P).set(torch.randn((T, P), generator=torch.Generator().manual_seed(3)))
    dW = a.new("dW", "inout", F32, P * E).set(0)
    db = a.new("db", "inout", F32, P).set(0)
    dg = a.new("dgamma", "inout", F32, P).set(0)
    dbt = a.new("dbeta", "inout", F32, P).set(0)
    bws = a.ws("bws", 4 * lib.t4r_pretrained_proj_bwd_ws_floats(T, E, P))
    a.seal()
    xh_before, out_before = xh.bits(), out.bits()
    rc = lib.t4r_pretrained_proj_bwd(_stream(), 3, img.ptr, ldp, V, ids.ptr, T, T // n_ids, dY.ptr, ld, col, gb.ptr, xh.ptr, rs.ptr,
                                     E, P, dW.ptr, db.ptr, dg.ptr, dbt.ptr, bws.ptr)
    assert rc == 0, lib.t4r_last_error()
    torch.cuda.synchronize()
    v = a.check()
    assert v is None, str(v)
    assert torch.equal(img.bits(), before) and torch.equal(xh.bits(), xh_before) and torch.equal(out.bits(), out_before)
    for buf in (dW, db, dg, dbt):
        assert buf.first_nonfinite() is None, buf.name
    assert float(dW.t.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ module level
NAME = "xlnet_mlm_pretrained_train"
PT = "heads.0.body.0.to_merge.pretrained_embedding_module."


def _fixture_model(d):
    L, Vt, E, P = int(d["meta/L"]), int(d["meta/V"]), int(d["meta/E"]), int(d["meta/P"])
    schema = tr.session_schema(Vt - 1, L) + tr.Schema([tr.ColumnSchema("item_vec", [tr.Tags.EMBEDDING, tr.Tags.LIST],
                                                                       embedding_dim=E)])
    inputs = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking="mlm", d_output=int(d["meta/d_model"]),
                                                    embedding_dim_default=int(d["meta/d_item"]), pretrained_output_dims=P,
                                                    normalizer="layer-norm")
    cfg = tr.XLNetConfig.build(dropout=0.0, d_model=int(d["meta/d_model"]), n_head=int(d["meta/n_head"]),
                               n_layer=int(d["meta/n_layer"]), total_seq_length=L)
    model = cfg.to_torch_model(inputs, tr.NextItemPredictionTask(weight_tying=True))
    sd, own = gu.section(d, "p/"), model.state_dict()
    missing = [k for k in sd if k not in own]
    assert not missing, missing
    with torch.no_grad():
        for k, v in sd.items():
            assert own[k].shape == v.shape, k
            own[k].copy_(v)
    assert all(PT + k in sd for k in ("projection.item_vec.weight", "post.feature_layer_norm.item_vec.bias"))
    return model.to(DEV)


def _close(a, b, rtol=1e-4, atol=5e-5, **kw):
    torch.testing.assert_close(a.detach().cpu(), b.detach().cpu(), rtol=rtol, atol=atol, **kw)


@pytest.mark.parametrize("form", ["dense", "attached"])
def test_fixture_replayed_through_the_module_mirror(form):
    d = gu.load(NAME)
    model = _fixture_model(d)
    x = {k[3:]: gu.t(v).to(DEV) for k, v in d.items() if k.startswith("in/")}
    pt = model.input_features.pretrained_module
    if form == "attached":
        pt.attach_table("item_vec", gu.t(d["table/item_vec"]).to(DEV))
        del x["item_vec"]
        assert not any("image" in k for k in model.state_dict())
    masking = model.input_features.masking
    masking.set_draws(gu.t(d["draw/bern"]).to(DEV).to(torch.uint8), gu.t(d["draw/j1"]).to(DEV), gu.t(d["draw/j2"]).to(DEV))
    out = model(x, training=True)
    model.input_features.check_ids()
    assert torch.equal(masking.masked_targets.cpu(), gu.t(d["out/masked_targets"]))
    _close(out["predictions"], gu.t(d["out/predictions"]))
    _close(out["loss"], gu.t(d["out/loss"]))
    out["loss"].backward()
    g = gu.section(d, "g/")
    named = dict(model.named_parameters())
    assert sum(k.startswith(PT) for k in g) == 4
    for k, ref in g.items():
        assert named[k].grad is not None, k
        _close(named[k].grad, ref, rtol=2e-4, atol=1e-4, msg=lambda m, k=k: f"{k}: {m}")


def test_fused_adam_step_moves_the_projection_and_not_the_image():
    d = gu.load(NAME)
    model = _fixture_model(d)
    pt = model.input_features.pretrained_module
    pt.attach_table("item_vec", gu.t(d["table/item_vec"]).to(DEV))
    x = {k[3:]: gu.t(v).to(DEV) for k, v in d.items() if k.startswith("in/") and k != "in/item_vec"}
    dense, tables = tr.flatten_model(model)
    assert any(n.startswith(PT) for n, _p, _o in dense.entries)
    opt = tr.FusedAdam([dense, tables], lr=1e-2)
    image = pt.table_image("item_vec")
    bits, w0 = image.view(torch.int16).clone(), pt.projection["item_vec"].weight.detach().clone()
    model(x, training=True)["loss"].backward()
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(pt.table_image("item_vec").view(torch.int16), bits)
    assert float((pt.projection["item_vec"].weight - w0).abs().max()) > 1e-3
    assert float((pt.post.feature_layer_norm["item_vec"].weight - gu.t(d["p/" + PT + "post.feature_layer_norm.item_vec.weight"])
                  .to(DEV)).abs().max()) > 1e-3


def test_mlm_inference_grid_runs():
    d = gu.load(NAME)
    model = _fixture_model(d)
    f = model.input_features
    x = {k[3:]: gu.t(v).to(DEV) for k, v in d.items() if k.startswith("in/")}
    dense_out = f(x, training=False, testing=False)
    B, L = x["item_id"].shape
    assert dense_out.shape == (B, L + 1, int(d["meta/d_model"]))
    f.pretrained_module.attach_table("item_vec", gu.t(d["table/item_vec"]).to(DEV))
    del x["item_vec"]
    _close(f(x, training=False, testing=False), dense_out, rtol=1e-5, atol=1e-6)


def _sum_block(agg="element-wise-sum", B=6, L=7, Vt=21, E=33, P=24):
    torch.manual_seed(3)
    cat = tr.SequenceEmbeddingFeatures({"item_id": (Vt, P)}, item_id="item_id")
    pt = tr.PretrainedEmbeddingFeatures(["vec"], E, pretrained_output_dims=P, normalizer="layer-norm")
    f = tr.TabularSequenceFeatures(cat, None, agg, pretrained_embedding_module=pt).to(DEV)
    table = torch.randn((Vt, E), device=DEV)
    ids = torch.randint(1, Vt, (B, L), device=DEV)
    ids[1, 4:] = 0
    x = {"item_id": ids, "vec": table.half().float()[ids]}
    return f, x, table


@pytest.mark.parametrize("agg", ["element-wise-sum", "element-wise-sum-item-multi"])
def test_element_wise_aggregations_with_equal_widths(agg):
    f, x, table = _sum_block(agg)
    pt = f.pretrained_module
    lin, ln = pt.projection["vec"], pt.post.feature_layer_norm["vec"]

    def torch_ref():
        e = f.item_embedding_table.weight.detach().double()[x["item_id"]]
        pw = [p.detach().double().requires_grad_(True) for p in (lin.weight, lin.bias, ln.weight, ln.bias)]
        r = torch.nn.functional.layer_norm(torch.nn.functional.linear(x["vec"].double(), pw[0], pw[1]), (24,), pw[2], pw[3], 1e-5)
        out = e + r if agg == "element-wise-sum" else e * r
        (out * out).sum().backward()
        return out, [p.grad for p in pw]

    ref, ref_g = torch_ref()
    grads = {}
    for form in ("dense", "attached"):
        f.zero_grad(set_to_none=True)
        xi = dict(x)
        if form == "attached":
            pt.attach_table("vec", table)
            del xi["vec"]
        out = f(xi, training=True)
        _close(out, ref.float(), rtol=1e-5, atol=1e-5)
        (out * out).sum().backward()
        grads[form] = [p.grad.clone() for p in (lin.weight, lin.bias, ln.weight, ln.bias)]
        for gk, gr in zip(grads[form], ref_g):
            _close(gk, gr.float(), rtol=1e-4, atol=1e-4)


def test_dense_and_device_resident_forms_agree(cases):
    """the same feature in both forms, to the forward bound: each within 4 x torch's fp32 error of float64"""
    for (E, P) in ((40, 24), (768, 64), (33, 1)):
        table, image, W, b, gamma, beta = cases[(E, P)]
        pt = tr.PretrainedEmbeddingFeatures(["v"], E, pretrained_output_dims=P, normalizer="layer-norm" if P > 1 else None)
        cat = tr.SequenceEmbeddingFeatures({"item_id": (V, 8)}, item_id="item_id")
        f = tr.TabularSequenceFeatures(cat, None, "concat", pretrained_embedding_module=pt).to(DEV)
        with torch.no_grad():
            pt.projection["v"].weight.copy_(W)
            pt.projection["v"].bias.copy_(b)
            if P > 1:
                pt.post.feature_layer_norm["v"].weight.copy_(gamma)
                pt.post.feature_layer_norm["v"].bias.copy_(beta)
        ids = _ids(15 * 9, 2).view(15, 9)
        ref = R.forward(image.cpu(), ids.reshape(-1), 135, W, b, gamma if P > 1 else None, beta if P > 1 else None)
        e_t = R.rel_err(R.forward(image.cpu(), ids.reshape(-1), 135, W, b, gamma if P > 1 else None, beta if P > 1 else None,
                                  dtype=torch.float32), ref)
        x = {"item_id": ids.to(DEV), "v": image.float()[ids.to(DEV)]}
        dense = f(x)[..., 8:].reshape(135, P).cpu()
        pt.attach_table("v", image.float())
        del x["v"]
        fused = f(x)[..., 8:].reshape(135, P).cpu()
        assert R.rel_err(fused, ref) <= 4 * e_t
        assert R.rel_err(dense, ref) <= 4 * e_t + 2e-7      # the general GEMM's own fp32 accumulation order
        assert float((dense - fused).abs().max()) <= (8 * e_t + 2e-7) * float(ref.abs().max())


def test_image_follows_the_module_and_stays_out_of_the_state_dict():
    pt = tr.PretrainedEmbeddingFeatures(["v"], 40, pretrained_output_dims=8).to(DEV)
    pt.attach_table("v", torch.randn(9, 40, device=DEV))
    assert not any("image" in k for k in pt.state_dict())
    img = pt.table_image("v")
    assert img.dtype == F16 and img.shape == (9, 40) and img.stride(0) == 48 and img.data_ptr() % 16 == 0
    pt.detach_table("v")
    assert pt.table_image("v") is None
