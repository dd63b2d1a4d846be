"""Host half of replaced-token detection: the float64 restatement (tests/rtd_head_restatement.py) against HuggingFace's
ElectraDiscriminatorPredictions + BCEWithLogitsLoss over the active positions, an fp32 evaluation of the chain inside the
restatement's bounds, six planted faults outside them, the twelfth C-ABI header (include/t4r_hip_rtd.h) against its ctypes
table, the size query and the argument limits (refused before any launch), the operators' fakes, the state-dict names and
every refusal of ReplacedTokenDetectionHead / RTDModel.  Nothing here needs a GPU."""
import ctypes
import math
import re

import pytest
import torch

import rtd_head_restatement as R
import transformers4rec_amd as tr
from transformers4rec_amd import _lib, ops, torch_ops

FOUR = ["t4r_rtd_head_bwd", "t4r_rtd_head_fwd", "t4r_rtd_head_supported", "t4r_rtd_head_ws_floats"]
GRADS = ("dx", "dW1", "db1", "dw2", "db2")


def _case(T, D, seed, scale=1.0, b2=0.3, n_off=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((T, D), generator=g) * scale
    W1 = torch.randn((D, D), generator=g) / math.sqrt(D) / scale
    b1 = torch.randn((D,), generator=g) * 0.1
    w2 = torch.randn((D,), generator=g) / math.sqrt(D)
    label = torch.rand((T,), generator=g) < 0.4
    active = torch.rand((T,), generator=g) < 0.7
    if n_off is not None:
        active = torch.arange(T) >= n_off
    return x, active, label, W1, b1, w2, torch.tensor([b2])


# ---------------------------------------------------------------------------------------------------------- the arithmetic
@pytest.mark.parametrize("act,name", [(R.GELU, "gelu"), (R.RELU, "relu")])
def test_restatement_equals_huggingface_electra_in_float64(act, name):
    electra = pytest.importorskip("transformers.models.electra.modeling_electra")
    from transformers import ElectraConfig

    B, L, D = 5, 7, 32
    x, active, label, W1, b1, w2, b2 = _case(B * L, D, 11)
    head = electra.ElectraDiscriminatorPredictions(ElectraConfig(hidden_size=D, hidden_act=name)).double()
    with torch.no_grad():
        head.dense.weight.copy_(W1), head.dense.bias.copy_(b1)
        head.dense_prediction.weight.copy_(w2.view(1, D)), head.dense_prediction.bias.copy_(b2)
    xh = x.double().view(B, L, D).requires_grad_(True)
    logits = head(xh)                                                     # [B, L]
    # ElectraForPreTraining.forward: the loss over attention_mask == 1
    on = active.view(B, L)
    loss = torch.nn.BCEWithLogitsLoss()(logits.view(-1, L)[on], label.view(B, L)[on].double())
    (loss * 1.7).backward()
    f = R.forward(x, active, label, W1, b1, w2, b2, act)
    r = R.backward(1.7, f, x, W1, w2, act)
    tol = dict(rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(f["z"], logits.detach().view(-1), **tol)
    torch.testing.assert_close(f["loss"], loss.detach(), **tol)
    torch.testing.assert_close(r["dx"], xh.grad.view(B * L, D), **tol)
    torch.testing.assert_close(r["dW1"], head.dense.weight.grad, **tol)
    torch.testing.assert_close(r["db1"], head.dense.bias.grad, **tol)
    torch.testing.assert_close(r["dw2"], head.dense_prediction.weight.grad.view(-1), **tol)
    torch.testing.assert_close(r["db2"], head.dense_prediction.bias.grad.view(()), **tol)
    # active None is every token
    f_all = R.forward(x, None, label, W1, b1, w2, b2, act)
    loss_all = torch.nn.BCEWithLogitsLoss()(logits.detach().view(-1), label.double())
    torch.testing.assert_close(f_all["loss"], loss_all, **tol)
    assert f_all["n"] == B * L


def test_restatement_with_no_active_token_is_zero_everywhere():
    x, _, label, W1, b1, w2, b2 = _case(9, 16, 3)
    f = R.forward(x, torch.zeros(9, dtype=torch.bool), label, W1, b1, w2, b2, R.GELU)
    r = R.backward(2.0, f, x, W1, w2, R.GELU)
    assert f["n"] == 0 and float(f["loss"]) == 0.0
    assert all(float(r[k].abs().max()) == 0.0 for k in GRADS)
    B = R.bounds(2.0, f, r, x, W1, b1, w2, b2, R.GELU)
    assert float(B["loss"]) == 0.0 and float(B["dx"].abs().max()) == 0.0


def _chain32(x, active, label, W1, b1, w2, b2, act, g):
    """the chain in fp32 torch with autograd (the composition of ordinary operators)"""
    x = x.clone().requires_grad_(True)
    W1, b1, w2, b2 = (t.clone().requires_grad_(True) for t in (W1, b1, w2, b2))
    a = torch.nn.functional.linear(x, W1, b1)
    h = torch.relu(a) if act == R.RELU else torch.nn.functional.gelu(a)
    z = h @ w2 + b2
    on = torch.ones_like(z, dtype=torch.bool) if active is None else active
    loss = torch.nn.functional.binary_cross_entropy_with_logits(z[on], label[on].float())
    (loss * g).backward()
    return {"a": a, "h": h, "z": z, "loss": loss, "dx": x.grad, "dW1": W1.grad, "db1": b1.grad, "dw2": w2.grad, "db2": b2.grad.view(())}


@pytest.mark.parametrize("act", [R.GELU, R.RELU])
@pytest.mark.parametrize("T,D,scale", [(65, 48, 1.0), (200, 128, 1e-3), (63, 64, 1e3)])
def test_fp32_torch_evaluation_stays_inside_the_bound(act, T, D, scale):
    x, active, label, W1, b1, w2, b2 = _case(T, D, 100 + T, scale)
    got = _chain32(x, active, label, W1, b1, w2, b2, act, 3.0)
    f = R.forward(x, active, label, W1, b1, w2, b2, act)
    r = R.backward(3.0, f, x, W1, w2, act)
    B = R.bounds(3.0, f, r, x, W1, b1, w2, b2, act)
    q = R.ratios({k: v.detach() for k, v in got.items()}, {**f, **r}, B)
    assert all(v <= 1.0 for v in q.values()), q


def _faulty(fault, x, active, label, W1, b1, w2, b2, act, g):
    """the restatement's chain in float64 with one planted fault"""
    x, W1, b1, w2, b2 = (t.double() for t in (x, W1, b1, w2, b2))
    y, on = label.double(), active.double()
    if fault == "label negated":
        y = 1.0 - y
    a = b1[None, :] + x @ W1.t()
    h = R.act_of(a, act)
    z = h @ w2 + (0.0 if fault == "b2 dropped" else b2[0])
    row = torch.clamp(z, min=0) - z * y + torch.log1p(torch.exp(-z.abs()))
    n = float(on.sum())
    div = float(x.shape[0]) if fault == "mean over T" else n
    w = torch.ones_like(on) if fault == "inactive rows counted" else on
    loss = (row * w).sum() / div
    dz = w * (g / div) * (torch.sigmoid(z) - y)
    da = dz[:, None] * w2[None, :] * R.act_grad_of(h if fault == "act' at h" else a, act)
    dx = da @ (W1.t() if fault == "W1 for W1^T" else W1)
    return {"z": z, "loss": loss, "dx": dx, "dW1": da.t() @ x, "db1": da.sum(0), "dw2": (dz[:, None] * h).sum(0), "db2": dz.sum()}


FAULTS = ["mean over T", "inactive rows counted", "label negated", "act' at h", "b2 dropped", "W1 for W1^T"]


@pytest.mark.parametrize("fault", [None] + FAULTS)
def test_planted_faults_exceed_the_bound(fault):
    T, D, act = 65, 48, R.GELU
    x, active, label, W1, b1, w2, b2 = _case(T, D, 7)
    assert 0 < int(active.sum()) < T
    f = R.forward(x, active, label, W1, b1, w2, b2, act)
    r = R.backward(3.0, f, x, W1, w2, act)
    B = R.bounds(3.0, f, r, x, W1, b1, w2, b2, act)
    q = R.ratios(_faulty(fault, x, active, label, W1, b1, w2, b2, act, 3.0), {**f, **r}, B)
    if fault is None:
        assert all(v <= 1e-6 for v in q.values()), q            # the harness itself: the same chain agrees
    else:
        assert max(q.values()) > 1.0, (fault, q)


# ---------------------------------------------------------------------------------------------------------- header and ABI
def test_rtd_header_library_and_prototypes_agree():
    lib = _lib.load()
    syms = _lib.header_symbols("t4r_hip_rtd.h")
    assert syms == FOUR
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/t4r_hip_rtd.h but not exported"
    text = open(_lib.header_path("t4r_hip_rtd.h")).read()
    assert "NaN" in text and "n = 0" in text                      # the stated difference from HF
    for entry in ("int t4r_rtd_head_fwd(void* stream", "int t4r_rtd_head_bwd(void* stream"):
        decl = text[: text.index(entry)]
        comment = decl[decl.rindex("/*"):]
        assert "replaces:" in comment, entry
    assert "ElectraDiscriminatorPredictions" in text and "BCEWithLogitsLoss" in text
    decls = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for word in ("at::", "torch", "Tensor", "std::", "c10"):
        assert word not in decls, f"{word} leaked into the C ABI"


def test_supported_and_ws_floats_are_pure_and_monotone():
    lib = _lib.load()
    ok = [D for D in range(0, 600) if lib.t4r_rtd_head_supported(D)]
    assert ok == list(range(16, 513, 16))
    assert lib.t4r_rtd_head_supported(-16) == 0
    f = lib.t4r_rtd_head_ws_floats
    assert f(0, 64) == 0 and f(-3, 64) == 0 and f(8, 0) == 0 and f(8, 24) == 0 and f(8, 528) == 0 and f(1 << 31, 64) == 0
    Ts = [1, 63, 64, 65, 127, 128, 129, 200, 20480, 51200, 1_000_000, (1 << 31) - 1]
    Ds = list(range(16, 513, 16))
    for D in Ds:
        got = [f(T, D) for T in Ts]
        assert got == [f(T, D) for T in Ts] and got == sorted(got) and got[0] >= D + 2 * D + 1 + D * D, (D, got)
    for T in Ts:
        got = [f(T, D) for D in Ds]
        assert got == sorted(got) and got[0] >= T * 16, (T, got)


BUF = ctypes.c_void_p(1 << 20)        # never dereferenced: every failing case below is refused before any launch


def _fwd(lib, T=4, D=16, act=0, x=BUF, label=BUF, loss=BUF):
    return lib.t4r_rtd_head_fwd(None, x, None, label, T, D, BUF, BUF, BUF, BUF, act, BUF, BUF, loss, BUF)


def _bwd(lib, T=4, D=16, act=0, dx=BUF):
    return lib.t4r_rtd_head_bwd(None, BUF, BUF, None, BUF, BUF, BUF, T, D, BUF, BUF, BUF, act, dx, None, None, None, None, BUF)


def test_limits_and_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    for call in (_fwd, _bwd):
        for kw, word in ((dict(D=0), b"D"), (dict(D=24), b"D"), (dict(D=528), b"D"), (dict(T=-1), b"T"), (dict(T=1 << 31), b"T"),
                         (dict(act=2), b"act"), (dict(act=-1), b"act")):
            assert call(lib, **kw) < 0, (call.__name__, kw)
            assert word in lib.t4r_last_error(), (call.__name__, kw, lib.t4r_last_error())
    assert _fwd(lib, x=None) < 0 and b"null" in lib.t4r_last_error()
    assert _fwd(lib, loss=None) < 0 and b"labels need" in lib.t4r_last_error()
    assert _bwd(lib, dx=None) < 0 and b"null" in lib.t4r_last_error()
    assert _fwd(lib, x=ctypes.c_void_p((1 << 20) + 2)) < 0 and b"aligned" in lib.t4r_last_error()
    assert _bwd(lib, dx=ctypes.c_void_p((1 << 20) + 2)) < 0 and b"aligned" in lib.t4r_last_error()
    # T = 0: nothing launches, nothing is looked at
    assert lib.t4r_rtd_head_fwd(None, None, None, None, 0, 16, None, None, None, None, 0, None, None, None, None) == 0
    assert lib.t4r_rtd_head_bwd(None, None, None, None, None, None, None, 0, 16, None, None, None, 0, None, None, None, None, None,
                                None) == 0
    x, W, v = torch.zeros(4, 16), torch.zeros(16, 16), torch.zeros(16)
    lab = torch.zeros(4, dtype=torch.bool)
    with pytest.raises(_lib.T4RHipError, match="GPU"):
        ops.rtd_head_fwd(x, None, lab, W, v, v, torch.zeros(1), 0)
    with pytest.raises(_lib.T4RHipError, match="GPU"):
        ops.rtd_head_bwd_(torch.ones(1), x, None, lab, torch.zeros(4), torch.ones(1, dtype=torch.int32), W, v, v, 0)


def test_operators_are_registered_and_their_fakes_give_the_shapes():
    assert {"rtd_head_fwd", "rtd_head_bwd"} <= set(torch_ops.OPERATORS)
    for name in ("rtd_head_fwd", "rtd_head_bwd"):
        assert str(getattr(torch.ops.t4r_hip, name).default._schema).startswith(f"t4r_hip::{name}(")
    m = lambda *s, **k: torch.empty(*s, device="meta", **k)     # noqa: E731
    z, n, loss = torch.ops.t4r_hip.rtd_head_fwd(m(35, 32), m(35, dtype=torch.bool), m(35, dtype=torch.bool), m(32, 32), m(32), m(32), m(1), 0)
    assert (z.shape, n.shape, n.dtype, loss.shape) == ((35,), (1,), torch.int32, (1,))
    z, n, loss = torch.ops.t4r_hip.rtd_head_fwd(m(35, 32), None, None, m(32, 32), m(32), m(1, 32), m(1), 1)
    assert (z.shape, n.shape, loss.shape) == ((35,), (0,), (0,))
    outs = torch.ops.t4r_hip.rtd_head_bwd(m(1), m(35, 32), None, m(35, dtype=torch.bool), m(35), m(1, dtype=torch.int32), m(32, 32),
                                          m(32), m(1, 32), 0)
    assert [tuple(o.shape) for o in outs] == [(35, 32), (32, 32), (32,), (1, 32), (1,)]


# ---------------------------------------------------------------------------------------------------------- modules
def test_head_state_dict_names_are_huggingfaces_and_a_checkpoint_loads():
    torch.manual_seed(0)
    head = tr.ReplacedTokenDetectionHead(64)
    sd = head.state_dict()
    assert list(sd) == ["dense.weight", "dense.bias", "dense_prediction.weight", "dense_prediction.bias"]
    assert [tuple(v.shape) for v in sd.values()] == [(64, 64), (64,), (1, 64), (1,)]
    assert float(sd["dense.bias"].abs().max()) == 0.0 and float(sd["dense_prediction.bias"].abs().max()) == 0.0
    assert 0.008 < float(sd["dense.weight"].std()) < 0.012
    electra = pytest.importorskip("transformers.models.electra.modeling_electra")
    from transformers import ElectraConfig

    hf = electra.ElectraDiscriminatorPredictions(ElectraConfig(hidden_size=64))
    head.load_state_dict(hf.state_dict(), strict=True)
    assert torch.equal(head.dense.weight, hf.dense.weight)
    from transformers4rec_amd.masking import hip_parameters

    assert {id(p) for p in hip_parameters(head)} == {id(p) for p in head.parameters()}


def test_head_refusals():
    for D in (0, 8, 24, 528):
        with pytest.raises(ValueError, match="hidden_size"):
            tr.ReplacedTokenDetectionHead(D)
    with pytest.raises(ValueError, match="hidden_act"):
        tr.ReplacedTokenDetectionHead(64, hidden_act="tanh")
    head = tr.ReplacedTokenDetectionHead(32)
    with pytest.raises(ValueError, match="hidden must be"):
        head(torch.zeros(2, 3, 16))
    with pytest.raises(ValueError, match="labels must be bool"):
        head(torch.zeros(2, 3, 32), labels=torch.zeros(2, 3))
    with pytest.raises(ValueError, match="active must be bool"):
        head(torch.zeros(2, 3, 32), labels=torch.zeros(2, 3, dtype=torch.bool), active=torch.zeros(2, 4, dtype=torch.bool))
    with pytest.raises(_lib.T4RHipError, match="GPU"):               # no CPU path
        head(torch.zeros(2, 3, 32), labels=torch.zeros(2, 3, dtype=torch.bool))


def _features(masking, L=6, V=50, D=64):
    return tr.TabularSequenceFeatures.from_schema(tr.session_schema(V, L), max_sequence_length=L, masking=masking, aggregation="concat",
                                                  embedding_dims={"item_id": D})


def _generator(masking="rtd", L=6, D=64):
    cfg = tr.XLNetConfig.build(dropout=0.0, d_model=D, n_head=2, n_layer=1, total_seq_length=L)
    return cfg.to_torch_model(_features(masking, L=L, D=D), tr.NextItemPredictionTask(weight_tying=True))


def _disc_block(L=6, D=64):
    return tr.TransformerBlock(tr.XLNetConfig.build(dropout=0.0, d_model=D, n_head=2, n_layer=1, total_seq_length=L))


def test_rtd_model_shares_the_item_table_and_names_its_parts():
    gen = _generator()
    model = tr.RTDModel(gen, _features(None), _disc_block())
    assert model.generator_loss_weight == 1.0 and model.discriminator_loss_weight == 50.0           # the reference args' defaults
    g_tab = gen.input_features.categorical_module.item_embedding_table
    assert model.discriminator_inputs.categorical_module.item_embedding_table is g_tab
    names = [n for n, _ in model.named_parameters()]
    assert sum(n.endswith("embedding_tables.item_id.weight") for n in names) == 1                    # once: the shared parameter
    assert {"head.dense.weight", "head.dense.bias", "head.dense_prediction.weight", "head.dense_prediction.bias"} <= set(names)
    own = tr.RTDModel(_generator(), _features(None), _disc_block(), share_item_embeddings=False)
    assert sum(n.endswith("embedding_tables.item_id.weight") for n, _ in own.named_parameters()) == 2


def test_rtd_model_refusals():
    with pytest.raises(ValueError, match="ReplacementLanguageModeling"):
        tr.RTDModel(_generator("mlm"), _features(None), _disc_block())
    with pytest.raises(ValueError, match="masking=None"):
        tr.RTDModel(_generator(), _features("mlm"), _disc_block())
    with pytest.raises(ValueError, match="differ in shape"):
        tr.RTDModel(_generator(), _features(None, D=32), _disc_block(D=32))
    tr.RTDModel(_generator(), _features(None, D=32), _disc_block(D=32), share_item_embeddings=False)         # allowed unshared
    with pytest.raises(ValueError, match="hidden size"):
        tr.RTDModel(_generator(), _features(None), _disc_block(), head=tr.ReplacedTokenDetectionHead(32))
    with pytest.raises(ValueError, match="generator must be a Model"):
        tr.RTDModel(_disc_block(), _features(None), _disc_block())
    multi = tr.XLNetConfig.build(dropout=0.0, d_model=64, n_head=2, n_layer=1, total_seq_length=6).to_torch_model(
        _features("rtd"), [tr.NextItemPredictionTask(weight_tying=True), tr.RegressionTask("dwell")])
    with pytest.raises(ValueError, match="exactly one NextItemPredictionTask"):
        tr.RTDModel(multi, _features(None), _disc_block())
    with pytest.raises(NotImplementedError, match="rtd_tied_generator"):
        tr.RTDModel(_generator(), _features(None), _disc_block(), rtd_tied_generator=True)
    with pytest.raises(NotImplementedError, match="rtd_use_batch_interaction"):
        tr.RTDModel(_generator(), _features(None), _disc_block(), rtd_use_batch_interaction=True)
    gen = _generator()
    gen.input_features.masking.sample_from_batch = True
    with pytest.raises(NotImplementedError, match="sample_from_batch"):
        tr.RTDModel(gen, _features(None), _disc_block())
    # autograd-visible gradient mode: refused at the training forward, before anything runs
    model = tr.RTDModel(_generator(), _features(None), _disc_block())
    tr.enable_autograd_gradients(model)
    with pytest.raises(NotImplementedError, match="autograd-visible"):
        model({"item_id": torch.ones(2, 6, dtype=torch.int64)}, training=True)
