"""Replaced-token detection on the GPU: the head kernels (csrc/rtd_head.hip, include/t4r_hip_rtd.h) against float64
(tests/rtd_head_restatement.py) under its per-element bounds, the output contract and its edge cases, bit-reproducibility, red
zones around every buffer with an exact workspace; the registered operators against the ctypes calls; the
ReplacedTokenDetectionHead module; and RTDModel (labels, the discriminator loss, linearity of the gradients in the two loss
weights, the shared item table under the fused optimizer, evaluation and inference equal to the generator's).

Every numeric test prints the largest observed error / bound ratio; with T4R_RATIO_LOG set to a path the maxima over the run
are also written there as JSON (profiles/rtd_head_margins.txt quotes them)."""
import atexit
import json
import math
import os

import pytest
import torch

import rtd_head_restatement as R
import transformers4rec_amd as tr
from abi_arena import FILLS, Arena
from transformers4rec_amd import _lib, ops, rng, torch_ops  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, I32, U8 = torch.float32, torch.int32, torch.uint8
U = R.U
OUT = ("z", "row", "loss", "dx", "dW1", "db1", "dw2", "db2")
PARAM_GRADS = ("dW1", "db1", "dw2", "db2")

RATIOS = {}


def _note(what, ratio):
    RATIOS[what] = max(RATIOS.get(what, 0.0), float(ratio))


@atexit.register
def _dump_ratios():
    path = os.environ.get("T4R_RATIO_LOG")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ws_floats(T, D):
    return _lib.load().t4r_rtd_head_ws_floats(T, D)


def raw_fwd(x, active, label, W1, b1, w2, b2, act, ws=None):
    """the C entry itself, every buffer the caller's (outputs pre-filled with NaN / -1) -> (z, n, loss, ws)"""
    T, D = x.shape
    nan = float("nan")
    z = torch.full((T,), nan, device=DEV)
    n = torch.full((1,), -1, device=DEV, dtype=I32)
    loss = torch.full((1,), nan, device=DEV)
    ws = torch.full((max(1, _ws_floats(T, D)),), nan, device=DEV) if ws is None else ws
    _lib.call("t4r_rtd_head_fwd", _stream(), _ptr(x), _ptr(active), _ptr(label), T, D, _ptr(W1), _ptr(b1), _ptr(w2), _ptr(b2), act,
              _ptr(z), _ptr(n), _ptr(loss), _ptr(ws))
    return z, n, loss, ws


def raw_bwd(g, x, active, label, z, n, W1, b1, w2, act, grads, dx=None, ws=None):
    """grads: (d_W1, d_b1, d_w2, d_b2), each a tensor or None -> dx"""
    T, D = x.shape
    nan = float("nan")
    dx = torch.full((T, D), nan, device=DEV) if dx is None else dx
    ws = torch.full((max(1, _ws_floats(T, D)),), nan, device=DEV) if ws is None else ws
    _lib.call("t4r_rtd_head_bwd", _stream(), _ptr(g), _ptr(x), _ptr(active), _ptr(label), _ptr(z), _ptr(n), T, D, _ptr(W1), _ptr(b1),
              _ptr(w2), act, _ptr(dx), *[_ptr(t) for t in grads], _ptr(ws))
    return dx


def _case(T, D, seed, scale=1.0, b2=0.3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((T, D), generator=g) * scale
    W1 = torch.randn((D, D), generator=g) / math.sqrt(D) / scale
    b1 = torch.randn((D,), generator=g) * 0.1
    w2 = torch.randn((D,), generator=g) / math.sqrt(D)
    label = torch.rand((T,), generator=g) < 0.4
    active = torch.rand((T,), generator=g) < 0.7
    return x, active, label, W1, b1, w2, torch.tensor([b2])


def _u8(m):
    return None if m is None else m.to(U8).to(DEV)


def _zeros(D):
    return [torch.zeros((D, D), device=DEV), torch.zeros((D,), device=DEV), torch.zeros((D,), device=DEV), torch.zeros((1,), device=DEV)]


def _run(case, act, g=3.0, grads=None):
    """forward + backward of one case through the C entries -> dict of the kernel's outputs (CPU tensors)"""
    x, active, label, W1, b1, w2, b2 = case
    T, D = x.shape
    xd, Wd, b1d, w2d, b2d = (t.to(DEV) for t in (x, W1, b1, w2, b2))
    ad, ld = _u8(active), _u8(label)
    z, n, loss, ws = raw_fwd(xd, ad, ld, Wd, b1d, w2d, b2d, act)
    rows = ws[:T].clone()
    grads = _zeros(D) if grads is None else grads
    dx = raw_bwd(torch.tensor([g], device=DEV), xd, ad, ld, z, n, Wd, b1d, w2d, act, grads)
    got = {"z": z, "row": rows, "loss": loss.view(()), "dx": dx, "n": n}
    got.update({k: (v.view(()) if k == "db2" else v) for k, v in zip(PARAM_GRADS, grads) if v is not None})
    return {k: v.cpu() for k, v in got.items()}


def _check(case, act, what, g=3.0, K=None):
    x, active, label, W1, b1, w2, b2 = case
    got = _run(case, act, g)
    f = R.forward(x, active, label, W1, b1, w2, b2, act)
    r = R.backward(g, f, x, W1, w2, act)
    B = R.bounds(g, f, r, x, W1, b1, w2, b2, act, K=K)
    assert int(got["n"]) == f["n"], what
    for k in OUT:
        assert bool(torch.isfinite(got[k]).all()), (what, k)
    want = {**f, **r}
    want["row"] = f["row"] * f["on"]                      # the workspace holds 0 at inactive tokens
    q = R.ratios({k: got[k] for k in OUT}, want, B)
    print(f"{what}: " + " ".join(f"{k}={v:.3f}" for k, v in q.items()))
    for k, v in q.items():
        _note(f"act{act} {k}", v)
    assert all(v <= 1.0 for v in q.values()), (what, q)
    return got, f, r


# ------------------------------------------------------------------------------------------------ kernel against float64
SHAPES = [(1, 16, 1.0), (63, 48, 1.0), (64, 64, 1e-3), (65, 128, 1e3), (200, 256, 1.0), (200, 64, 1.0), (65, 256, 1e-3),
          (129, 80, 1.0), (130, 512, 1.0)]


@pytest.mark.parametrize("act", [R.GELU, R.RELU])
@pytest.mark.parametrize("T,D,scale", SHAPES)
def test_kernel_against_the_restatement(T, D, scale, act):
    _check(_case(T, D, 1000 * T + D, scale), act, f"T={T} D={D} scale={scale} act={act}")


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_saturated_logits_are_finite_and_inside_the_bound(sign):
    _, f, _ = _check(_case(65, 64, 5, b2=80.0 * sign), R.GELU, f"saturated b2={80.0 * sign}")
    assert float(f["z"].abs().min()) > 70.0


@pytest.mark.parametrize("which", ["all true", "all false", "active NULL", "one session all padding"])
def test_label_and_mask_edge_cases(which):
    x, active, label, W1, b1, w2, b2 = _case(70, 48, 9)
    if which == "all true":
        label = torch.ones_like(label)
    elif which == "all false":
        label = torch.zeros_like(label)
    elif which == "active NULL":
        active = None
    else:
        active = active.clone()
        active[20:30] = False               # B = 7, L = 10: session 2 is all padding
    got, f, _ = _check((x, active, label, W1, b1, w2, b2), R.RELU if which == "all true" else R.GELU, which)
    if which == "one session all padding":
        assert float(got["dx"][20:30].abs().max()) == 0.0
    if active is not None:
        assert float(got["dx"][~active].abs().max()) == 0.0 and bool(torch.isfinite(got["z"][~active]).all())


def test_no_active_token_gives_zero_loss_and_zero_gradients():
    x, _, label, W1, b1, w2, b2 = _case(70, 48, 10)
    active = torch.zeros(70, dtype=torch.bool)
    pre = [torch.full_like(t, 1.25) for t in _zeros(48)]
    got = _run((x, active, label, W1, b1, w2, b2), R.GELU, grads=pre)
    assert int(got["n"]) == 0 and float(got["loss"]) == 0.0
    assert float(got["dx"].abs().max()) == 0.0
    assert all(bool((got[k] == 1.25).all()) for k in PARAM_GRADS)            # nothing was added
    assert bool(torch.isfinite(got["z"]).all())


def test_inference_writes_the_logits_only():
    x, _, _, W1, b1, w2, b2 = _case(65, 48, 12)
    z_t = _run(_case(65, 48, 12), R.GELU)["z"]
    z, n, loss, _ = raw_fwd(x.to(DEV), None, None, W1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV), R.GELU)
    assert torch.equal(z.cpu(), z_t) and int(n) == -1 and bool(torch.isnan(loss).all())
    _lib.call("t4r_rtd_head_fwd", _stream(), _ptr(x.to(DEV)), None, None, 65, 48, _ptr(W1.to(DEV)), _ptr(b1.to(DEV)), _ptr(w2.to(DEV)),
              _ptr(b2.to(DEV)), R.GELU, _ptr(z), None, None, None)            # n_active, loss and ws may be NULL


def _bits(d):
    return {k: v.view(I32) if v.dtype == F32 else v for k, v in d.items()}


def test_rerun_is_bit_equal_and_prefilled_gradients_are_added_to():
    case = _case(200, 80, 13)
    a, b = _run(case, R.GELU), _run(case, R.GELU)
    for k in a:
        assert torch.equal(_bits(a)[k], _bits(b)[k]), k
    pre = [torch.randn(t.shape, generator=torch.Generator().manual_seed(i)).to(DEV) for i, t in enumerate(_zeros(80))]
    keep = [p.clone() for p in pre]
    c = _run(case, R.GELU, grads=pre)
    for k, p in zip(PARAM_GRADS, keep):
        assert torch.equal(c[k], (p.cpu().view(a[k].shape) + a[k])), k         # ONE add of the same sum
    assert torch.equal(c["dx"], a["dx"])


def test_null_gradient_pointers_are_accepted():
    case = _case(130, 48, 14)
    full = _run(case, R.RELU)
    for skip in range(4):
        grads = _zeros(48)
        grads[skip] = None
        got = _run(case, R.RELU, grads=grads)
        assert PARAM_GRADS[skip] not in got and torch.equal(got["dx"], full["dx"])
        for k in PARAM_GRADS:
            assert k not in got or torch.equal(got[k], full[k]), (skip, k)
    got = _run(case, R.RELU, grads=[None] * 4)
    assert torch.equal(got["dx"], full["dx"])


def test_a_base_address_off_by_four_bytes_gives_the_same_bits():
    x, active, label, W1, b1, w2, b2 = _case(130, 80, 15)
    T, D = x.shape
    ref = _run((x, active, label, W1, b1, w2, b2), R.GELU)

    def off(t):                                    # the same values one float past a 16-byte boundary
        buf = torch.empty(t.numel() + 1, device=DEV, dtype=t.dtype)
        buf[1:].copy_(t.reshape(-1))
        v = buf[1:].view(t.shape)
        assert v.data_ptr() % 16 == 4
        return v

    xd, Wd, b1d, w2d, b2d = (off(t.to(DEV)) for t in (x, W1, b1, w2, b2))
    ad, ld = _u8(active), _u8(label)
    ws = off(torch.full((_ws_floats(T, D),), float("nan"), device=DEV))
    z, n, loss, _ = raw_fwd(xd, ad, ld, Wd, b1d, w2d, b2d, R.GELU, ws=ws)
    grads = [off(t) for t in _zeros(D)]
    dx = raw_bwd(torch.tensor([3.0], device=DEV), xd, ad, ld, z, n, Wd, b1d, w2d, R.GELU, grads, dx=off(torch.empty(T, D, device=DEV)),
                 ws=off(torch.full((_ws_floats(T, D),), float("nan"), device=DEV)))
    got = {"z": z, "loss": loss.view(()), "dx": dx, **{k: v.view(ref[k].shape) for k, v in zip(PARAM_GRADS, grads)}}
    for k, v in got.items():
        assert torch.equal(v.cpu().view(I32), ref[k].view(I32)), k


def test_a_token_alone_gives_the_bits_it_has_inside_a_batch():
    x, _, label, W1, b1, w2, b2 = _case(70, 128, 16)
    T = x.shape[0]
    batch = _run((x, None, label, W1, b1, w2, b2), R.GELU, g=float(T))          # g / n = 1 exactly, as alone with g = 1
    for t in (0, 37, 69):
        alone = _run((x[t:t + 1], None, label[t:t + 1], W1, b1, w2, b2), R.GELU, g=1.0)
        assert torch.equal(alone["z"].view(I32), batch["z"][t:t + 1].view(I32)), t
        assert torch.equal(alone["dx"].view(I32), batch["dx"][t:t + 1].view(I32)), t


@pytest.mark.parametrize("fill", FILLS)
def test_red_zones_and_exact_workspace(fill):
    T, D, act = 130, 48, R.GELU
    x, active, label, W1, b1, w2, b2 = _case(T, D, 17)
    ar = Arena(fill, device=DEV)
    bx = ar.new("x", "in", F32, (T, D)).set(x)
    ba = ar.new("active", "in", U8, (T,)).set(active.to(U8))
    bl = ar.new("label", "in", U8, (T,)).set(label.to(U8))
    bW = ar.new("W1", "in", F32, (D, D)).set(W1)
    bb1 = ar.new("b1", "in", F32, (D,)).set(b1)
    bw2 = ar.new("w2", "in", F32, (D,)).set(w2)
    bb2 = ar.new("b2", "in", F32, (1,)).set(b2)
    bz = ar.new("z", "out", F32, (T,))
    bn = ar.new("n_active", "out", I32, (1,))
    bloss = ar.new("loss", "out", F32, (1,))
    ws1 = ar.ws("ws fwd", 4 * _ws_floats(T, D))
    ar.seal()
    _lib.call("t4r_rtd_head_fwd", _stream(), bx.ptr, ba.ptr, bl.ptr, T, D, bW.ptr, bb1.ptr, bw2.ptr, bb2.ptr, act, bz.ptr, bn.ptr,
              bloss.ptr, ws1.ptr)
    torch.cuda.synchronize()
    assert ar.check() is None, str(ar.check())
    assert ar.nonfinite() is None, ar.nonfinite()
    bg = ar.new("g", "in", F32, (1,)).set(3.0)
    bdx = ar.new("dx", "out", F32, (T, D))
    bdW = ar.new("d_W1", "inout", F32, (D, D)).set(0.0)
    bdb1 = ar.new("d_b1", "inout", F32, (D,)).set(0.0)
    bdw2 = ar.new("d_w2", "inout", F32, (D,)).set(0.0)
    bdb2 = ar.new("d_b2", "inout", F32, (1,)).set(0.0)
    ws2 = ar.ws("ws bwd", 4 * _ws_floats(T, D))
    ar.seal()
    _lib.call("t4r_rtd_head_bwd", _stream(), bg.ptr, bx.ptr, ba.ptr, bl.ptr, bz.ptr, bn.ptr, T, D, bW.ptr, bb1.ptr, bw2.ptr, act,
              bdx.ptr, bdW.ptr, bdb1.ptr, bdw2.ptr, bdb2.ptr, ws2.ptr)
    torch.cuda.synchronize()
    assert ar.check() is None, str(ar.check())
    assert ar.nonfinite() is None, ar.nonfinite()
    ref = _run((x, active, label, W1, b1, w2, b2), act)
    assert torch.equal(bz.win.cpu(), ref["z"]) and torch.equal(bdx.win.cpu(), ref["dx"]) and torch.equal(bdW.win.cpu(), ref["dW1"])
    assert int(bn.win) == int(ref["n"]) and torch.equal(bloss.win.cpu().view(()), ref["loss"])


# ------------------------------------------------------------------------------------------------ operators and module
def test_registered_operators_give_the_bits_of_the_ctypes_calls():
    x, active, label, W1, b1, w2, b2 = _case(130, 64, 18)
    ref = _run((x, active, label, W1, b1, w2, b2), R.GELU, g=0.75)
    xd, ad, ld, Wd, b1d, w2d, b2d = x.to(DEV), active.to(DEV), label.to(DEV), W1.to(DEV), b1.to(DEV), w2.to(DEV).view(1, -1), b2.to(DEV)
    z, n, loss = torch.ops.t4r_hip.rtd_head_fwd(xd, ad, ld, Wd, b1d, w2d, b2d, R.GELU)
    assert torch.equal(z.cpu(), ref["z"]) and int(n) == int(ref["n"]) and torch.equal(loss.cpu().view(()), ref["loss"])
    zi, ni, li = torch.ops.t4r_hip.rtd_head_fwd(xd, None, None, Wd, b1d, w2d, b2d, R.GELU)
    assert torch.equal(zi, z) and ni.shape == (0,) and li.shape == (0,)
    outs = torch.ops.t4r_hip.rtd_head_bwd(torch.tensor([0.75], device=DEV), xd, ad, ld, z, n, Wd, b1d, w2d, R.GELU)
    for k, v in zip(("dx",) + PARAM_GRADS, outs):
        assert torch.equal(v.cpu().view(ref[k].shape), ref[k]), k
    assert outs[3].shape == (1, 64)
    with pytest.raises(ValueError, match="multiple of 16"):
        ops.rtd_head_fwd(torch.zeros(4, 24, device=DEV), None, None, torch.zeros(24, 24, device=DEV), torch.zeros(24, device=DEV),
                         torch.zeros(24, device=DEV), torch.zeros(1, device=DEV), 0)


@pytest.mark.parametrize("act_name", ["gelu", "relu"])
def test_head_module_matches_the_restatement(act_name):
    B, L, D = 9, 7, 48
    act = ops.RTD_ACT[act_name]
    torch.manual_seed(3)
    head = tr.ReplacedTokenDetectionHead(D, hidden_act=act_name).to(DEV)
    with torch.no_grad():
        head.dense.weight.mul_(10.0), head.dense.bias.normal_(0, 0.1), head.dense_prediction.weight.mul_(10.0)
        head.dense_prediction.bias.fill_(0.2)
    x, active, label, *_ = _case(B * L, D, 19)
    W1, b1 = head.dense.weight.detach().cpu(), head.dense.bias.detach().cpu()
    w2, b2 = head.dense_prediction.weight.detach().cpu().view(-1), head.dense_prediction.bias.detach().cpu()
    xd = x.view(B, L, D).to(DEV).requires_grad_(True)
    out = head(xd, labels=label.view(B, L).to(DEV), active=active.view(B, L).to(DEV))
    assert set(out) == {"loss", "logits"} and out["loss"].shape == () and out["logits"].shape == (B, L)
    (out["loss"] * 2.0).backward()
    f = R.forward(x, active, label, W1, b1, w2, b2, act)
    r = R.backward(2.0, f, x, W1, w2, act)
    Bd = R.bounds(2.0, f, r, x, W1, b1, w2, b2, act)
    got = {"z": out["logits"].detach().view(-1), "loss": out["loss"].detach(), "dx": xd.grad.view(B * L, D), "dW1": head.dense.weight.grad,
           "db1": head.dense.bias.grad, "dw2": head.dense_prediction.weight.grad.view(-1), "db2": head.dense_prediction.bias.grad.view(())}
    q = R.ratios(got, {**f, **r}, Bd)
    print(f"module {act_name}: {q}")
    assert all(v <= 1.0 for v in q.values()), q
    # inference: the same logits, no loss; a frozen parameter keeps .grad untouched
    with torch.no_grad():
        inf = head(xd.detach())
    assert inf["loss"] is None and torch.equal(inf["logits"], out["logits"])
    before = head.dense.weight.grad.clone()
    head.dense.weight.requires_grad_(False)
    xd2 = x.view(B, L, D).to(DEV).requires_grad_(True)
    head(xd2, labels=label.view(B, L).to(DEV), active=active.view(B, L).to(DEV))["loss"].backward()
    assert torch.equal(head.dense.weight.grad, before) and torch.equal(xd2.grad * 2.0, xd.grad)


# ------------------------------------------------------------------------------------------------ RTDModel
L_, V_, D_ = 6, 50, 64


def _features(masking, D=D_):
    return tr.TabularSequenceFeatures.from_schema(tr.session_schema(V_, L_), max_sequence_length=L_, masking=masking, aggregation="concat",
                                                  embedding_dims={"item_id": D})


def _rtd_model(body="xlnet", share=True, seed=0):
    torch.manual_seed(seed)
    cfg = tr.XLNetConfig.build(dropout=0.0, d_model=D_, n_head=2, n_layer=1, total_seq_length=L_)
    gen = cfg.to_torch_model(_features("rtd"), tr.NextItemPredictionTask(weight_tying=True))
    dcfg = cfg if body == "xlnet" else tr.BertConfig.build(d_model=D_, n_head=2, n_layer=1, total_seq_length=L_)
    model = tr.RTDModel(gen, _features(None), tr.TransformerBlock(dcfg), share_item_embeddings=share).to(DEV).train()
    with torch.no_grad():                      # logits of a useful size: the initial head gives |z| ~ 1e-3
        model.head.dense.weight.mul_(20.0), model.head.dense_prediction.weight.mul_(20.0)
    return model


def _batch(B=16, seed=1):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, V_ + 1, (B, L_), generator=g)
    lens = torch.randint(2, L_ + 1, (B,), generator=g)
    ids[torch.arange(L_)[None, :] >= lens[:, None]] = 0
    return {"item_id": ids.to(DEV)}


@pytest.mark.parametrize("body", ["xlnet", "bert"])
def test_rtd_model_labels_and_discriminator_loss(body):
    model = _rtd_model(body)
    x = _batch()
    seen = {}
    model.discriminator_inputs.register_forward_pre_hook(lambda m, args: seen.__setitem__("ids", args[0]["item_id"].clone()))
    model.discriminator_block.register_forward_hook(lambda m, args, out: seen.__setitem__("h", out.detach().clone()))
    out = model(x, training=True)
    assert set(out) == {"loss", "generator_loss", "discriminator_loss", "labels", "predictions", "discriminator_logits", "discriminator_labels"}
    ids, corrupted, dl = x["item_id"], seen["ids"], out["discriminator_labels"]
    targets = model.generator.input_features.masking.masked_targets
    assert dl.dtype == torch.bool and dl.shape == ids.shape and bool((targets != 0).any())
    assert torch.equal(dl, corrupted != ids)                                   # False wherever the drawn item is the original
    assert not bool(dl[targets == 0].any()) and torch.equal(corrupted[targets == 0], ids[targets == 0])
    assert bool(((corrupted >= 0) & (corrupted <= V_)).all())
    # the discriminator's loss and logits: the restatement over the body's output and the returned labels
    head = model.head
    h = seen["h"].cpu().view(-1, D_)
    W1, b1 = head.dense.weight.detach().cpu(), head.dense.bias.detach().cpu()
    w2, b2 = head.dense_prediction.weight.detach().cpu().view(-1), head.dense_prediction.bias.detach().cpu()
    active = (ids != 0).cpu().view(-1)
    f = R.forward(h, active, dl.cpu().view(-1), W1, b1, w2, b2, R.GELU)
    Bd = R.bounds(1.0, f, None, h, W1, b1, w2, b2, R.GELU)
    q = R.ratios({"z": out["discriminator_logits"].detach().view(-1), "loss": out["discriminator_loss"].detach()}, f, Bd)
    print(f"RTDModel {body}: {q}")
    assert all(v <= 1.0 for v in q.values()), q
    total = 1.0 * out["generator_loss"].detach() + 50.0 * out["discriminator_loss"].detach()
    assert abs(float(out["loss"].detach()) - float(total)) <= 4 * U * abs(float(total))
    out["loss"].backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.head.parameters())


def _grads(model, x, state, wg, wd):
    rng.set_rng_state(model, state)
    for p in model.parameters():
        p.grad = None
    model.generator_loss_weight, model.discriminator_loss_weight = wg, wd
    model(x, training=True)["loss"].backward()
    torch.cuda.synchronize()
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("share", [True, False])
def test_gradients_are_linear_in_the_two_loss_weights(share):
    """Every kernel on the backward path is linear in the upstream gradient, so grads(wg, wd) and wg grads(1, 0) + wd grads(0, 1)
    differ by rounding only.  The bound is 1024 u (sum |terms| + the tensor's largest sum |terms|) with terms = wg |grads(1, 0)|,
    wd |grads(0, 1)|: about 16 chained contractions of length <= 4 D = 256 lie between the loss and the farthest parameter, each
    within (K + 2) u of ITS sum |terms| in fp32 -- or 4 u per product in the body's two-way fp16 split --, and a contraction's
    sum |terms| is bounded by the tensor's largest entry, not by the element's own, which is why the tensor's maximum is in."""
    model = _rtd_model("xlnet", share)
    x = _batch()
    state = rng.get_rng_state(model)
    wg, wd = 0.7, 50.0
    both, g10, g01 = _grads(model, x, state, wg, wd), _grads(model, x, state, 1.0, 0.0), _grads(model, x, state, 0.0, 1.0)
    again = _grads(model, x, state, wg, wd)
    tables = [k for k in both if k.endswith("embedding_tables.item_id.weight")]
    assert len(tables) == (1 if share else 2)
    assert any(k.startswith("head.") for k in both) and any(k.startswith("discriminator_block.") for k in both)
    worst = 0.0
    for k, gb in both.items():
        assert torch.equal(gb, again[k]), k                                    # the replayed step: the same bits
        a, b = g10.get(k), g01.get(k)
        a = torch.zeros_like(gb) if a is None else a
        b = torch.zeros_like(gb) if b is None else b
        terms = wg * a.double().abs() + wd * b.double().abs()
        bound = 1024 * U * (terms + terms.max())
        err = (gb.double() - (wg * a.double() + wd * b.double())).abs()
        if float(terms.max()) > 0:
            worst = max(worst, float((err / bound.clamp(min=1e-300)).max()))
        assert bool((err <= bound).all()), (k, float((err / bound.clamp(min=1e-300)).max()))
    if share:                                   # both passes reach the one table
        k = tables[0]
        assert float(g10[k].abs().max()) > 0 and float(g01[k].abs().max()) > 0
    print(f"linearity share={share}: worst ratio {worst:.4f}")


def test_fused_adam_moves_the_shared_table_once():
    model = _rtd_model("xlnet", True)
    x = _batch()
    dense, tables = tr.flatten_model(model)
    lr = 1e-2
    opt = tr.FusedAdam([b for b in (dense, tables) if b is not None], lr=lr)
    tab = model.generator.input_features.categorical_module.item_embedding_table.weight
    assert model.discriminator_inputs.categorical_module.item_embedding_table.weight is tab
    assert sum(p is tab for p in model.parameters()) == 1
    before = tab.detach().clone()
    head_before = model.head.dense.weight.detach().clone()
    model(x, training=True)["loss"].backward()
    opt.step()
    torch.cuda.synchronize()
    moved = (tab.detach() - before).abs()
    # Adam's first step moves an element by lr |g| / (|g| + eps) <= lr: once, not twice
    assert 0.5 * lr < float(moved.max()) <= lr * (1 + 1e-5), float(moved.max())
    assert float((model.head.dense.weight.detach() - head_before).abs().max()) > 0.5 * lr


def _same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(p, q) for p, q in zip(a, b))
    a = a.materialize() if hasattr(a, "materialize") else a
    b = b.materialize() if hasattr(b, "materialize") else b
    return torch.equal(a, b) if torch.is_tensor(a) else a == b


def test_evaluation_and_inference_are_the_generators():
    model = _rtd_model("xlnet").eval()
    x = _batch()
    with torch.no_grad():
        assert _same(model(x, testing=True), model.generator(x, testing=True))
        assert _same(model(x), model.generator(x))
