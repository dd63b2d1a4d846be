"""`continuous_projection` on the GPU: the first-layer kernels (csrc/cont_proj.hip, include/t4r_hip_contproj.h) against float64
(tests/cont_proj_restatement.py) under the FMA-chain bounds, accumulation, exact-zero units, the dpre output, bit-reproducibility
and red zones around every buffer; the module path against the reference's fixtures (tests/golden/xlnet_mlm_contproj*_train.npz,
tools/make_contproj_golden.py); and two input blocks without a projection held to the bits they gave before the feature existed
(tests/golden/contproj_regression.npz, tools/make_contproj_regression.py)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import cont_proj_restatement as R
import golden_utils as gu
import transformers4rec_amd as tr
from abi_arena import FILLS, Arena
from transformers4rec_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32

# (B, L, C, P): a pruned cross of (B, L) in {(1,1), (3,7), (5,33), (64,20)}, C in {1, 3, 16, 33, 64}, P in {1, 4, 6, 64, 100, 1024}
# that reaches every kernel form: 64 or 128 outputs per workgroup, each column-group count of the backward, one and several
# output tiles, one and several token tiles, T below / at / above a tile, P % 4 != 0
CASES = [(1, 1, 1, 1), (1, 1, 3, 4), (3, 7, 3, 6), (3, 7, 16, 64), (3, 7, 64, 1024), (5, 33, 1, 100), (5, 33, 33, 100),
         (5, 33, 64, 4), (5, 33, 16, 1024), (64, 20, 3, 64), (64, 20, 16, 100), (64, 20, 33, 6), (64, 20, 1, 1024)]
BLOCKS = lambda P: [(0, P), (8, P + 12), (3, P + 5)]      # (col, ld) of the gradient block  # noqa: E731


def _case(B, L, C, P):
    """columns (a mix of [B, L] and [B]; trailing positions of a session are zero = padding), W, b as torch.nn.Linear draws
    them, with one unit (P // 2, when P > 1) whose weights and bias are exactly zero"""
    g = torch.Generator().manual_seed(B * 1000 + L * 100 + C * 10 + P)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    m = (torch.arange(L)[None] < lens[:, None]).float()
    flags = [C > 1 and c % 3 == 1 for c in range(C)]
    xs = [torch.randn((B,), generator=g) if f else torch.randn((B, L), generator=g) * m for f in flags]
    if C > 1:
        xs[1][B // 2] = 0.0             # a per-session zero as well
    bound = 1.0 / C ** 0.5
    W = (torch.rand((P, C), generator=g) * 2 - 1) * bound
    b = (torch.rand((P,), generator=g) * 2 - 1) * bound
    if P > 1:
        W[P // 2] = 0.0
        b[P // 2] = 0.0
    return xs, flags, W, b


def _dev(ts):
    return [t.to(DEV) for t in ts]


@pytest.fixture(scope="module")
def cases():
    out = {}
    for c in CASES:
        xs, flags, W, b = _case(*c)
        y64, ybound = R.forward(xs, flags, c[1], W, b)
        out[c] = dict(xs=xs, flags=flags, W=W, b=b, y64=y64, ybound=ybound)
    return out


# ------------------------------------------------------------------------------------------------ kernel forward
@pytest.mark.parametrize("B,L,C,P", CASES)
def test_forward_against_float64(cases, B, L, C, P):
    k = cases[(B, L, C, P)]
    y = ops.cont_proj_fwd(_dev(k["xs"]), k["flags"], k["W"].to(DEV), k["b"].to(DEV), T=B * L)
    assert y.shape == (B * L, P) and y.is_contiguous()
    y = y.cpu()
    err = (y.double() - k["y64"]).abs()
    slack = err / k["ybound"].clamp_min(1e-300)
    print(f"forward B={B} L={L} C={C} P={P}: worst error / bound {float(slack.max()):.3f}, max |y| {float(y.abs().max()):.3f}")
    assert bool((err <= k["ybound"]).all()), float(slack.max())
    assert float(y.min()) >= 0.0
    # a position whose columns are all zero (padding) comes out as relu(b), exactly
    X = R.stack(k["xs"], k["flags"], L)
    pad = (X == 0).all(dim=1)
    if bool(pad.any()):
        assert torch.equal(y[pad], torch.relu(k["b"]).expand(int(pad.sum()), P))
    if P > 1:
        assert float(y[:, P // 2].abs().max()) == 0.0


def test_forward_bits_do_not_depend_on_the_launch_shape(cases):
    k = cases[(64, 20, 16, 100)]
    xs, W, b = _dev(k["xs"]), k["W"].to(DEV), k["b"].to(DEV)
    full = ops.cont_proj_fwd(xs, k["flags"], W, b, T=1280).view(64, 20, 100)
    part = ops.cont_proj_fwd([x[5:8].contiguous() for x in xs], k["flags"], W, b, T=60).view(3, 20, 100)
    assert torch.equal(part, full[5:8])
    narrow = ops.cont_proj_fwd(xs, k["flags"], W[:37].contiguous(), b[:37].contiguous(), T=1280).view(64, 20, 37)
    assert torch.equal(narrow, full[..., :37])


# ------------------------------------------------------------------------------------------------ kernel backward
def _run_bwd(k, T, P, dY, col, ld, d_w=None, d_b=None, want_dpre=False):
    C = len(k["xs"])
    wide = torch.full((T, ld), 3.25, device=DEV)
    wide[:, col:col + P] = dY.to(DEV)
    d_w = torch.zeros((P, C), device=DEV) if d_w is None else d_w
    d_b = torch.zeros(P, device=DEV) if d_b is None else d_b
    dpre = ops.cont_proj_bwd_(wide, col, _dev(k["xs"]), k["flags"], k["W"].to(DEV), k["b"].to(DEV), d_w, d_b, want_dpre=want_dpre)
    return d_w, d_b, dpre


@pytest.mark.parametrize("B,L,C,P", CASES)
def test_backward_against_float64(cases, B, L, C, P):
    k = cases[(B, L, C, P)]
    T = B * L
    y_dev = ops.cont_proj_fwd(_dev(k["xs"]), k["flags"], k["W"].to(DEV), k["b"].to(DEV), T=T).cpu()
    mask = y_dev > 0                                    # the device's own forward: no case hangs on a sign inside the rounding band
    dY = torch.randn((T, P), generator=torch.Generator().manual_seed(T + P))
    dW64, db64, bW, bb = R.gradients(k["xs"], k["flags"], L, dY, mask)
    for col, ld in BLOCKS(P):
        d_w, d_b, dpre = _run_bwd(k, T, P, dY, col, ld, want_dpre=True)
        eW, eb = (d_w.cpu().double() - dW64).abs(), (d_b.cpu().double() - db64).abs()
        print(f"backward B={B} L={L} C={C} P={P} col={col} ld={ld}: d_w error / bound "
              f"{float((eW / bW.clamp_min(1e-300)).max()):.3f}, d_b {float((eb / bb.clamp_min(1e-300)).max()):.3f}")
        assert bool((eW <= bW).all()) and bool((eb <= bb).all()), (col, ld)
        assert torch.equal(dpre.cpu(), dY * mask), (col, ld)            # the masked gradient: the input's bits or zero
        if P > 1:       # a unit with zero weights and zero bias has output exactly 0: no gradient (torch's ReLU at 0)
            assert float(d_w[P // 2].abs().max()) == 0.0 and float(d_b[P // 2]) == 0.0
    # two runs: the same bits; without dpre: the same bits
    again = _run_bwd(k, T, P, dY, col, ld)
    assert torch.equal(again[0], d_w) and torch.equal(again[1], d_b) and again[2] is None
    # accumulated: the sum over the tokens is formed first, then added once to what the buffers held
    pre_w = torch.full((P, C), 0.5, device=DEV) + torch.arange(C, device=DEV) * 0.125
    pre_b = torch.full((P,), -0.25, device=DEV)
    acc = _run_bwd(k, T, P, dY, col, ld, d_w=pre_w.clone(), d_b=pre_b.clone())
    assert torch.equal(acc[0], pre_w + d_w) and torch.equal(acc[1], pre_b + d_b)


def test_a_dropped_token_would_be_caught(cases):
    """the margin of the bound at the largest T used here: one token's share of d_b is far above it"""
    k = cases[(64, 20, 16, 100)]
    dY = torch.randn((1280, 100), generator=torch.Generator().manual_seed(1))
    mask = k["y64"] > 0
    _dW, _db, _bW, bb = R.gradients(k["xs"], k["flags"], 20, dY, mask)
    share = (dY * mask).abs().max(dim=0).values.double()
    live = share > 0
    assert float((bb[live] / share[live]).max()) < 0.05


# ------------------------------------------------------------------------------------------------ red zones
def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("fill", FILLS, ids=["zeros", "ones"])
@pytest.mark.parametrize("B,L,C,P", [(3, 7, 3, 6), (5, 33, 33, 100), (3, 7, 64, 1024), (64, 20, 16, 100), (1, 1, 1, 1)])
def test_red_zones_around_every_buffer(cases, fill, B, L, C, P):
    lib = _lib.load()
    k = cases[(B, L, C, P)]
    T, col, pad = B * L, 3, 2
    a = Arena(fill, DEV, capacity=24 << 20)
    xb = [a.new(f"x{c}", "in", F32, x.numel()).set(x) for c, x in enumerate(k["xs"])]
    Wb = a.new("W", "in", F32, P * C).set(k["W"])
    bb = a.new("b", "in", F32, P).set(k["b"])
    out = a.new("out", "out", F32, T * P)
    a.seal()
    ptrs, _kp = _lib.ptr_array([x.ptr for x in xb])
    flags, _kf = _lib.int_array([int(f) for f in k["flags"]])
    rc = lib.t4r_cont_proj_fwd(_stream(), ptrs, flags, T, L, C, P, Wb.ptr, bb.ptr, out.ptr)
    assert rc == 0, lib.t4r_last_error()
    torch.cuda.synchronize()
    v = a.check()
    assert v is None, str(v)
    assert a.nonfinite() is None
    want = ops.cont_proj_fwd(_dev(k["xs"]), k["flags"], k["W"].to(DEV), k["b"].to(DEV), T=T)
    assert torch.equal(out.t.view(T, P), want)
    # ---- backward: the gradient block inside wider rows, the exact workspace
    ld = col + P + pad
    dY = torch.randn((T, P), generator=torch.Generator().manual_seed(3))
    dyb = a.new("dout", "in", F32, (T, ld), col=col, width=P).set(dY)
    dW = a.new("d_w", "inout", F32, P * C).set(0)
    db = a.new("d_b", "inout", F32, P).set(0)
    dpre = a.new("dpre", "out", F32, T * P)
    ws = a.ws("ws", 4 * lib.t4r_cont_proj_bwd_ws_floats(T, C, P))
    a.seal()
    out_before = out.bits()
    rc = lib.t4r_cont_proj_bwd(_stream(), dyb.ptr, ld, col, ptrs, flags, T, L, C, P, Wb.ptr, bb.ptr, dW.ptr, db.ptr, dpre.ptr, ws.ptr)
    assert rc == 0, lib.t4r_last_error()
    torch.cuda.synchronize()
    v = a.check()
    assert v is None, str(v)
    assert a.nonfinite() is None and torch.equal(out.bits(), out_before)
    assert torch.equal(dpre.t.view(T, P).cpu(), dY * (want.cpu() > 0))
    if bool((want > 0).any()):
        assert float(db.t.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ module level
NAMES = ["xlnet_mlm_contproj_train", "xlnet_mlm_contproj2_train"]
CP = "heads.0.body.0.to_merge.continuous_module."
CATS, CONTS = (("category", 7),), ("price", "age_days", "hour")


def _fixture_model(d):
    L, Vt = int(d["meta/L"]), int(d["meta/V"])
    dims = [int(v) for v in d["meta/dims"]]
    inputs = tr.TabularSequenceFeatures.from_schema(
        tr.session_schema(Vt - 1, L, CATS, CONTS), max_sequence_length=L, masking="mlm", aggregation=str(d["meta/aggregation"]),
        d_output=int(d["meta/d_model"]), embedding_dims={"item_id": int(d["meta/d_item"]), "category": int(d["meta/d_cat"])},
        continuous_projection=dims if len(dims) > 1 else dims[0])
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
    assert sum(k.startswith(CP) for k in sd) == 2 * len(dims)
    return model.to(DEV)


def _close(a, b, rtol=1e-4, atol=5e-5, **kw):
    torch.testing.assert_close(a.detach().cpu(), b.detach().cpu(), rtol=rtol, atol=atol, **kw)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_replayed_through_the_module_mirror(name):
    d = gu.load(name)
    model = _fixture_model(d)
    x = {k[3:]: gu.t(v).to(DEV) for k, v in d.items() if k.startswith("in/")}
    masking = model.input_features.masking
    masking.set_draws(gu.t(d["draw/bern"]).to(DEV).to(torch.uint8), gu.t(d["draw/j1"]).to(DEV), gu.t(d["draw/j2"]).to(DEV))
    cap = {}
    model.input_features.register_forward_hook(lambda m, i, o: cap.__setitem__("emb", o.detach().clone()))
    out = model(x, training=True)
    model.input_features.check_ids()
    assert torch.equal(masking.masked_targets.cpu(), gu.t(d["out/masked_targets"]))
    _close(cap["emb"], gu.t(d["out/inputs_embeds"]))
    _close(out["predictions"], gu.t(d["out/predictions"]))
    _close(out["loss"], gu.t(d["out/loss"]))
    out["loss"].backward()
    g = gu.section(d, "g/")
    named = dict(model.named_parameters())
    assert sum(k.startswith(CP) for k in g) == 2 * len(d["meta/dims"])
    for k, ref in g.items():
        assert named[k].grad is not None, k
        _close(named[k].grad, ref, rtol=2e-4, atol=1e-4, msg=lambda m, k=k: f"{k}: {m}")


def _block(agg="concat", dims=(12, 16), B=6, L=7, Vt=21, masking=None, per_session=False):
    """an input block without the d_output projection: its output is the aggregate itself"""
    torch.manual_seed(3)
    width = dims[-1] if agg != "concat" else 8
    f = tr.TabularSequenceFeatures.from_schema(
        tr.session_schema(Vt - 1, L, (), CONTS), max_sequence_length=L, aggregation=agg, embedding_dim_default=width,
        continuous_projection=list(dims), masking=masking).to(DEV)
    g = torch.Generator().manual_seed(4)
    lens = torch.randint(2, L + 1, (B,), generator=g)
    m = torch.arange(L)[None] < lens[:, None]
    x = {"item_id": (torch.randint(1, Vt, (B, L), generator=g) * m).to(DEV)}
    for i, n in enumerate(CONTS):
        x[n] = (torch.randn((B,), generator=g) if per_session and i == 1 else torch.randn((B, L), generator=g) * m).to(DEV)
    return f, x, lens


def _block_float64(f, x, agg, grad=False):
    """the aggregate in float64 with torch autograd -> (out [B, L, W], [parameters])"""
    cont = f.continuous_module
    B, L = x["item_id"].shape
    ps = [p.detach().double().requires_grad_(grad) for lin in cont.layers for p in (lin.weight, lin.bias)]
    cols = [x[n].double() if x[n].ndim == 2 else x[n].double()[:, None].expand(B, L) for n in cont.names]
    h = torch.stack(cols, dim=-1)
    for i in range(len(cont.layers)):
        h = torch.relu(torch.nn.functional.linear(h, ps[2 * i], ps[2 * i + 1]))
    e = f.item_embedding_table.weight.detach().double()[x["item_id"]]
    if agg == "concat":
        out = torch.cat([h, e], dim=-1)            # sorted names: continuous_projection < item_id
    else:
        out = e + h if agg == "element-wise-sum" else e * h
    return out, ps


@pytest.mark.parametrize("agg,dims,per_session", [("concat", (24,), False), ("concat", (12, 6), True), ("concat", (9, 5), False), ("element-wise-sum", (12, 16), True),
                                                  ("element-wise-sum-item-multi", (12, 16), False), ("element-wise-sum-item-multi", (16,), False)])
def test_aggregations_against_float64_autograd(agg, dims, per_session):
    f, x, _lens = _block(agg, dims, per_session=per_session)
    ref, ps = _block_float64(f, x, agg, grad=True)
    (ref * ref).sum().backward()
    out = f(x, training=True)
    _close(out, ref.float(), rtol=1e-5, atol=1e-5)
    (out * out).sum().backward()
    got = [p.grad for lin in f.continuous_module.layers for p in (lin.weight, lin.bias)]
    for gk, p in zip(got, ps):
        _close(gk, p.grad.float(), rtol=1e-4, atol=1e-4)
    first = [g.clone() for g in got]
    f.zero_grad(set_to_none=True)
    out = f(x, training=True)
    (out * out).sum().backward()
    for a, lin_p in zip(first, [p for lin in f.continuous_module.layers for p in (lin.weight, lin.bias)]):
        assert torch.equal(a, lin_p.grad)           # the whole block's gradients: the same bits from run to run


def test_mlm_inference_grid_and_evaluation_agree_with_float64():
    f, x, lens = _block("concat", (12, 20), masking="mlm")
    B, L = x["item_id"].shape
    ref, _ps = _block_float64(f, x, "concat")
    W = ref.shape[-1]
    infer = f(x, training=False, testing=False)
    assert infer.shape == (B, L + 1, W)
    evalu = f(x, training=False, testing=True)
    assert evalu.shape == (B, L, W)
    keep = ~f.masking.mask_schema.cpu()            # evaluation masks the last item of each session: every other position is the aggregate
    valid = torch.arange(L)[None] < lens[:, None]
    assert int((keep & valid).sum()) > B
    _close(evalu.cpu()[keep & valid], ref.float().cpu()[keep & valid], rtol=1e-5, atol=1e-5)
    _close(infer.cpu()[:, :L][valid], ref.float().cpu()[valid], rtol=1e-5, atol=1e-5)


def test_projecting_a_block_that_is_on_the_device_already():
    torch.manual_seed(1)
    f = tr.TabularSequenceFeatures.from_schema(tr.session_schema(20, 7, (), CONTS), max_sequence_length=7, aggregation="concat",
                                               embedding_dim_default=8, d_output=16).to(DEV)
    f.project_continuous_features([12, 8])
    assert all(p.device.type == "cuda" for p in f.parameters()) and f.projection_module[0][0].weight.shape == (16, 16)
    _f, x, _lens = _block("concat", (12, 8))
    ref, _ps = _block_float64(f, x, "concat")
    lin = f.projection_module[0][0]
    want = torch.relu(torch.nn.functional.linear(ref, lin.weight.detach().double(), lin.bias.detach().double()))
    _close(f(x), want.float(), rtol=1e-5, atol=1e-5)


def test_swap_noise_still_acts_on_the_raw_columns():
    torch.manual_seed(0)
    f = tr.TabularSequenceFeatures.from_schema(tr.session_schema(20, 7, (), CONTS), max_sequence_length=7, aggregation="concat",
                                               embedding_dim_default=8, continuous_projection=16,
                                               pre=tr.StochasticSwapNoise(replacement_prob=0.5)).to(DEV)
    _f, x, _lens = _block("concat", (16,))
    f.eval()
    quiet = f(x)
    f.train()
    noisy = f(x, training=True)
    assert noisy.shape == quiet.shape and not torch.equal(noisy, quiet) and bool(torch.isfinite(noisy).all())


# ------------------------------------------------------------------------------------------------ regression guards
@pytest.mark.parametrize("case", ["plain", "soft"])
def test_blocks_without_a_projection_keep_their_bits(case):
    spec = importlib.util.spec_from_file_location("make_contproj_regression", os.path.join(ROOT, "tools", "make_contproj_regression.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rec = np.load(os.path.join(ROOT, "tests", "golden", mod.NAME + ".npz"))
    want = {k[len(case) + 1:]: torch.from_numpy(rec[k]) for k in rec.files if k.startswith(case + "/")}
    got = mod.run(tr, mod.CASES[case], DEV)
    assert sorted(got) == sorted(want) and len(want) > 4
    for k in want:
        assert torch.equal(got[k], want[k]), k
