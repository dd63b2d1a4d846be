"""GPT-2 and BERT bodies in TRAINING mode (dropout on) against the CPU oracle taking the same decisions (GPU).

The kernels under these bodies are checked one launch at a time in tests/test_kernels_gpu.py, each against a mask exported from
the device for that launch.  This file checks how transformers4rec_amd/transformer_hf.py COMPOSES them: which dropout sites exist,
which (offset, layer, site) counter each one draws from, the order of dropout against LayerNorm and the residual add, BERT's two
rates, and whether every backward re-draws the mask its own forward used.  The other side is written independently of that file:

  * the site list and the arithmetic are HF's, restated in oracle/t4r_oracle.py (gpt2_model_dropout / bert_model_dropout) and pinned
    against the installed HF models in .train() by tests/test_oracle_vs_hf.py (CPU);
  * the masks are the integer restatement of the device streams, oracle/device_rng.py (gpt2_dropout_masks / bert_dropout_masks):
    nothing is read back from the device but the results.

Tolerances.  Bodies alone: the layer-test bounds of tests/test_kernels_gpu.py (output rtol 2e-5 / atol 3e-5, gradients rtol 1e-4 /
atol 5e-4).  Whole steps: the bounds of tests/test_round6_gpu.py (loss and logits 1e-4, gradients rtol 2e-3 / atol 2e-6).  Every
comparison prints the share of its tolerance it used (`pytest -s`); DESIGN.md lists the figures measured on an MI355X.
"""
import pytest
import torch

import device_rng as R
import golden_utils as gu
import t4r_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRE = "heads.0.body.1.transformer."
OUT_TOL = dict(rtol=2e-5, atol=3e-5)        # tests/test_kernels_gpu.py: one layer's output
GRAD_TOL = dict(rtol=1e-4, atol=5e-4)       # ... and its gradients
STEP_TOL = dict(rtol=2e-3, atol=2e-6)       # tests/test_round6_gpu.py: gradients of one training step
STEP_ABS = 1e-4                             # ... its loss and logits


@pytest.fixture(scope="module")
def ops():
    import build_c
    from transformers4rec_amd import ops as _ops

    build_c.build()
    return _ops


def cu(t):
    return t.to(DEV).contiguous()


def used(got, want, rtol, atol):
    """the largest |got - want| / (atol + rtol |want|): <= 1 passes assert_close"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float(((got - want).abs() / (atol + rtol * want.abs())).max())


def close(got, want, name, log=None, rtol=1e-4, atol=1e-5):
    if log is not None:
        log[name] = used(got, want, rtol, atol)
    torch.testing.assert_close(got.detach().cpu().float(), want.detach().cpu().float(), rtol=rtol, atol=atol,
                               msg=lambda m: f"{name}: {m}")


def report(tag, log):
    grads = {k: v for k, v in log.items() if k != "output"}
    worst = max(grads, key=grads.get)
    head = f"output {log['output']:.3f} of its tolerance, " if "output" in log else ""
    print(f"\n[{tag}] {head}{len(grads)} gradients, the worst: {worst} at {grads[worst]:.3f} of its tolerance")


# ------------------------------------------------------------------------------------------ the bodies alone
def grad_names(arch, n_layer):
    """every parameter of the body that the forward uses (HF state_dict names), spelled out: none may drop out of the comparison"""
    if arch == "gpt2":
        names = ["wpe.weight", "ln_f.weight", "ln_f.bias"]
        for i in range(n_layer):
            names += [f"h.{i}.{m}.{w}" for m in ("ln_1", "attn.c_attn", "attn.c_proj", "ln_2", "mlp.c_fc", "mlp.c_proj")
                      for w in ("weight", "bias")]
        assert len(names) == 3 + 12 * n_layer
    else:
        names = ["embeddings.position_embeddings.weight", "embeddings.token_type_embeddings.weight",
                 "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"]
        for i in range(n_layer):
            names += [f"encoder.layer.{i}.{m}.{w}"
                      for m in ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense",
                                "attention.output.LayerNorm", "intermediate.dense", "output.dense", "output.LayerNorm")
                      for w in ("weight", "bias")]
        assert len(names) == 4 + 16 * n_layer
    return names


def make_body(arch, L, D, n, rates, seed, n_layer=2):
    """GPT2Model / BertModel built directly, every parameter random (weights 0.1 N(0,1), LayerNorm weights around 1, biases
    non-zero: the builders' 0.01 and zero biases would hide a missing bias gradient), on the device in .train(), `seed` assigned"""
    import transformers4rec_amd as tr

    if arch == "gpt2":
        cfg = tr.GPT2Config.build(D, n, n_layer, total_seq_length=L, dropout=rates[0])
    else:
        cfg = tr.BertConfig.build(D, n, n_layer, total_seq_length=L, hidden_dropout_prob=rates[0],
                                  attention_probs_dropout_prob=rates[1])
        assert cfg.intermediate_size == 3072 and cfg.layer_norm_eps == 0.03
    model = cfg.to_huggingface_torch_model()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            ln = ("ln_" in name or "LayerNorm" in name) and name.endswith("weight")
            p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g) if ln else 0.1 * torch.randn(p.shape, generator=g))
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model.to(DEV).train()
    model.seed = seed
    return model, sd


def body_masks(arch, B, L, D, n, rates, seed, offset, n_layer=2):
    if arch == "gpt2":
        return R.gpt2_dropout_masks(B, L, D, n, n_layer, rates[0], seed=seed, offset=offset)
    return R.bert_dropout_masks(B, L, D, n, n_layer, rates[0], rates[1], seed=seed, offset=offset)


def oracle_body(arch, sd, x, dout, n, masks, rates, key_len=None, dtype=torch.float32):
    """-> (output, d inputs_embeds, {state_dict name: gradient}) of the oracle body in training mode"""
    leaves = {k: v.to(dtype).clone().requires_grad_() for k, v in sd.items()}
    xo = x.to(dtype).clone().requires_grad_()
    if arch == "gpt2":
        out = O.gpt2_model_dropout(xo, O.gpt2_params_from_state(leaves), n, 1e-5, masks, rates[0], key_len=key_len)
    else:
        out = O.bert_model_dropout(xo, O.bert_params_from_state(leaves), n, 0.03, masks, rates[0], rates[1], key_len=key_len)
    if dout is None:
        return out.detach(), None, None
    out.backward(dout.to(dtype))
    return out.detach(), xo.grad, {k: v.grad for k, v in leaves.items() if v.grad is not None}


def device_forward(model, x, key_len=None):
    xd = cu(x).requires_grad_()
    (h,) = model(inputs_embeds=xd, key_len=None if key_len is None else cu(key_len))
    return xd, h


def device_backward(model, xd, h, dout):
    for p in model.parameters():
        p.grad = None
    xd.grad = None
    h.backward(cu(dout))
    torch.cuda.synchronize()
    return xd.grad.cpu(), {k: p.grad.cpu() for k, p in model.named_parameters() if p.grad is not None}


def compare_body(tag, arch, got, want, n_layer=2, rows=None):
    """output, d inputs_embeds (on `rows` if given) and EVERY parameter gradient"""
    (h, dx, grads), (h_ref, dx_ref, grads_ref) = got, want
    names = grad_names(arch, n_layer)
    assert sorted(grads_ref) == sorted(names), "the oracle's own parameter list"
    assert sorted(grads) == sorted(names), f"parameters with a gradient on the device: {sorted(set(grads) ^ set(names))}"
    if arch == "bert":
        assert not any(k.startswith("pooler.") for k in grads)          # HF computes it, TransformerBlock drops it: no gradient
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    log = {}
    close(sel(h), sel(h_ref), "output", log, **OUT_TOL)
    close(sel(dx), sel(dx_ref), "d inputs_embeds", log, **GRAD_TOL)
    for k in names:
        close(grads[k], grads_ref[k], k, log, **GRAD_TOL)
    assert len(log) == 2 + len(names)
    report(tag, log)


BODY_CASES = [            # the smallest shapes that reach each attention path of csrc/mha.hip
    ("gpt2", 3, 20, 64, 4, (0.3, 0.3)),       # short kernels, d_head 16
    ("gpt2", 2, 50, 128, 2, (0.3, 0.3)),      # short, d_head 64
    ("gpt2", 2, 130, 96, 4, (0.3, 0.3)),      # general kernels: L > 128, d_head 24
    ("bert", 3, 20, 64, 4, (0.1, 0.1)),       # short
    ("bert", 2, 33, 128, 4, (0.1, 0.1)),      # d_head 32, odd L
    ("bert", 2, 130, 48, 2, (0.1, 0.1)),      # general
    ("bert", 3, 20, 64, 4, (0.1, 0.3)),       # the two rates cannot be exchanged unnoticed
    ("bert", 2, 130, 48, 2, (0.1, 0.3)),
]


def _inputs(B, L, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, L, D, generator=g), torch.randn(B, L, D, generator=g)


@pytest.mark.parametrize("arch,B,L,D,n,rates", BODY_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_body_training_forward_backward_vs_oracle(ops, arch, B, L, D, n, rates):
    """one training forward + backward of the body: output, d inputs_embeds and every parameter gradient"""
    seed = 1000 + L + D
    model, sd = make_body(arch, L, D, n, rates, seed)
    x, dout = _inputs(B, L, D, seed + 1)
    xd, h = device_forward(model, x)
    assert model._drop_offset == 1
    dx, grads = device_backward(model, xd, h, dout)
    masks = body_masks(arch, B, L, D, n, rates, seed, offset=1)
    want = oracle_body(arch, sd, x, dout, n, masks, rates)
    with torch.no_grad():             # the masks mattered: the eval-mode oracle is elsewhere
        plain = (O.gpt2_model(x, O.gpt2_params_from_state(sd), n, 1e-5) if arch == "gpt2" else
                 O.bert_model(x, O.bert_params_from_state(sd), n, 0.03))
    assert float((plain - want[0]).abs().max()) > 1e-1
    compare_body(f"body {arch} B{B} L{L} D{D} n{n} p{rates}", arch, (h.detach().cpu(), dx, grads), want)


@pytest.mark.parametrize("arch,rates", [("gpt2", (0.3, 0.3)), ("bert", (0.1, 0.1))])
def test_body_training_with_the_padding_mask(ops, arch, rates):
    """dropout on AND the opt-in padding mask (key_len).  Compared on the valid positions, as
    tests/test_oracle_vs_hf.py::test_gpt2_bert_padding_mask_restatement_matches_hf does and for its reason (a padded query row is
    arithmetic noise in both implementations); the upstream gradient is zero on the padded positions, so that the parameter
    gradients are defined by the valid ones alone."""
    B, L, D, n, seed = 4, 20, 64, 4, 77
    key_len = torch.tensor([20, 1, 10, 3], dtype=torch.int32)
    valid = torch.arange(L)[None] < key_len[:, None]
    model, sd = make_body(arch, L, D, n, rates, seed)
    x, dout = _inputs(B, L, D, seed + 1)
    dout = dout * valid[..., None]
    xd, h = device_forward(model, x, key_len)
    dx, grads = device_backward(model, xd, h, dout)
    masks = body_masks(arch, B, L, D, n, rates, seed, offset=1)
    want = oracle_body(arch, sd, x, dout, n, masks, rates, key_len=key_len)
    if arch == "bert":                # (a causal body never lets a valid query see a padded key: the mask changes nothing there)
        unmasked = oracle_body(arch, sd, x, None, n, masks, rates)[0]
        assert float((unmasked - want[0])[valid].abs().max()) > 1e-2
    compare_body(f"body {arch} padding mask", arch, (h.detach().cpu(), dx, grads), want, rows=valid)


@pytest.mark.parametrize("arch,rates", [("gpt2", (0.3, 0.3)), ("bert", (0.1, 0.3))])
def test_the_forward_counter(ops, arch, rates):
    """`_drop_offset`: one step per TRAINING forward, none per eval forward; every backward re-draws the masks of ITS forward"""
    B, L, D, n, seed = 3, 20, 64, 4, 31
    model, sd = make_body(arch, L, D, n, rates, seed)
    x, dout = _inputs(B, L, D, seed + 1)
    xd1, h1 = device_forward(model, x)
    assert model._drop_offset == 1
    model.eval()
    with torch.no_grad():
        (e1,) = model(inputs_embeds=cu(x))
        (e2,) = model(inputs_embeds=cu(x))
    assert model._drop_offset == 1                       # an eval forward draws nothing
    assert torch.equal(e1, e2)
    plain = (O.gpt2_model(x, O.gpt2_params_from_state(sd), n, 1e-5) if arch == "gpt2" else
             O.bert_model(x, O.bert_params_from_state(sd), n, 0.03))
    close(e1, plain, "eval output", **OUT_TOL)
    model.train()
    xd2, h2 = device_forward(model, x)
    assert model._drop_offset == 2
    assert float((h1.detach() - h2.detach()).abs().max()) > 1e-1      # other masks
    want = {off: oracle_body(arch, sd, x, dout, n, body_masks(arch, B, L, D, n, rates, seed, offset=off), rates) for off in (1, 2)}
    # the backward of the second forward, then -- with the counter at 2 -- the backward of the FIRST: each with its own masks
    dx2, g2 = device_backward(model, xd2, h2, dout)
    compare_body(f"counter {arch} offset 2", arch, (h2.detach().cpu(), dx2, g2), want[2])
    dx1, g1 = device_backward(model, xd1, h1, dout)
    compare_body(f"counter {arch} offset 1, backward run after the second forward", arch, (h1.detach().cpu(), dx1, g1), want[1])
    assert model._drop_offset == 2


# ------------------------------------------------------------------------------------------ whole training steps
def make_step_model(arch, V, L, D, n, n_layer, rates=None):
    """the module mirror as the builders make it (their initialisation and, unless `rates` is given, their dropout rates: GPT-2 0.3,
    BERT 0.1 / 0.1), tied weights"""
    import transformers4rec_amd as tr

    schema = tr.session_schema(V, L)
    torch.manual_seed(0)
    inputs = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking="clm" if arch == "gpt2" else "mlm",
                                                    embedding_dim_default=D)
    kw = {} if rates is None else dict(hidden_dropout_prob=rates[0], attention_probs_dropout_prob=rates[1])
    cfg = (tr.GPT2Config if arch == "gpt2" else tr.BertConfig).build(D, n, n_layer, total_seq_length=L, **kw)
    model = cfg.to_torch_model(inputs, tr.NextItemPredictionTask(weight_tying=True))
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model.to(DEV).train()
    return schema, model, sd


def step_oracle_params(arch, sd, dtype=torch.float32):
    p = gu.oracle_params({"p/" + k: v.numpy() for k, v in sd.items()}, requires_grad=True, dtype=dtype)
    leaves = {k: v.to(dtype).clone().requires_grad_() for k, v in sd.items() if k.startswith(PRE)}
    p["body"] = (O.gpt2_params_from_state if arch == "gpt2" else O.bert_params_from_state)(leaves, PRE)
    return p, leaves


STEP_CASES = [
    ("gpt2", 20, 64, 4, None), ("gpt2", 130, 96, 4, None),
    ("bert", 20, 64, 4, None), ("bert", 130, 48, 2, None),
    ("bert", 20, 64, 4, (0.1, 0.3)),      # the builder's 0.1 / 0.1 cannot tell the two rates apart: one case where they differ
]


@pytest.mark.parametrize("arch,L,D,n,rates", STEP_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_gpt2_bert_dropout_step_vs_oracle(ops, arch, L, D, n, rates):
    """one training step of the module mirror (lookup -> CLM / MLM input masking -> body with dropout -> label rows -> tied
    full-softmax head -> CE) against the CPU oracle taking the same decisions: CLM targets from the rule, MLM targets and every
    dropout mask from the restatement of the device streams alone."""
    import transformers4rec_amd as tr

    B, V, NL = 24, 3000, 2
    schema, model, sd = make_step_model(arch, V, L, D, n, NL, rates)
    body, masking = model.transformer_block.transformer, model.input_features.masking
    masking.seed, body.seed = 77, 78
    if arch == "gpt2":
        rates_used = (body.config.resid_pdrop,) * 2
        assert rates_used == (0.3, 0.3)
    else:
        rates_used = (body.config.hidden_dropout_prob, body.config.attention_probs_dropout_prob)
        assert rates_used == (rates or (0.1, 0.1))
    data = tr.random_data_from_schema(schema, B, L, seed=5)
    out = model({k: v.to(DEV) for k, v in data.items()}, training=True)
    out["loss"].backward()
    torch.cuda.synchronize()
    assert body._drop_offset == 1
    ids = data["item_id"]
    if arch == "gpt2":
        mask, labels = O.clm_targets(ids, True, False)
    else:
        mask, labels = R.mlm_targets_train_device(ids, 77, 0, 0.15)
    assert torch.equal(masking.mask_schema.cpu(), mask) and torch.equal(masking.masked_targets.cpu(), labels)
    masks = body_masks(arch, B, L, D, n, rates_used, 78, offset=1, n_layer=NL)
    cfg_o = dict(n_head=n, item="item_id", masking="clm" if arch == "gpt2" else "mlm", body=arch)
    drop_of = lambda r, m: (r[0] if arch == "gpt2" else r, m)
    p, leaves = step_oracle_params(arch, sd)
    ref = O.session_forward(p, cfg_o, data, mask, labels, True, False, drop=drop_of(rates_used, masks))
    ref["loss"].backward()
    logits = out["predictions"].detach().cpu()
    assert torch.equal(out["labels"].cpu(), ref["labels"]), "labels"
    dl = abs(float(out["loss"].detach()) - float(ref["loss"].detach()))
    dp = float((logits - ref["logits"].detach()).abs().max())
    tag = f"step {arch} L{L} D{D} n{n} p{rates_used}"
    print(f"\n[{tag}] loss {float(ref['loss'].detach()):.6f}: |d loss| {dl:.2e}, max |d logits| {dp:.2e} over {tuple(logits.shape)}")
    assert dl < STEP_ABS, f"loss: |d| {dl:.3e}"
    assert dp < STEP_ABS, f"logits: max |d| {dp:.3e}"
    # sensitivity: the same oracle step with ONE composition mistake misses the device's logits by > 100 x the bound
    swapped = dict(masks, layers=[dict(lm) for lm in masks["layers"]])
    swapped["layers"][NL - 1]["attn_out"], swapped["layers"][NL - 1]["ff_out"] = (masks["layers"][NL - 1]["ff_out"],
                                                                                  masks["layers"][NL - 1]["attn_out"])
    variants = {"one layer's attn_out and ff_out masks exchanged": drop_of(rates_used, swapped),
                "offset 2": drop_of(rates_used, body_masks(arch, B, L, D, n, rates_used, 78, offset=2, n_layer=NL))}
    if rates_used[0] != rates_used[1]:
        variants["the two rates exchanged in the scales"] = drop_of(rates_used[::-1], masks)
    with torch.no_grad():
        for name, drop in variants.items():
            miss = float((O.session_forward(p, cfg_o, data, mask, labels, True, False, drop=drop)["logits"] - logits).abs().max())
            print(f"[{tag}] {name}: misses the device's logits by {miss:.2e}")
            assert miss > 100 * STEP_ABS, f"{name}: the oracle step is not sensitive to it ({miss:.3e})"
    log = {}
    close(model.input_features.item_embedding_table.weight.grad, p["tables"]["item_id"].grad, "item table", log, **STEP_TOL)
    close(masking.masked_item_embedding.grad, p["masked_item_embedding"].grad, "masked_item_embedding", log, **STEP_TOL)
    names = grad_names(arch, NL)                 # the position table, every block's / layer's weights, the LayerNorms
    got = {k: q.grad for k, q in body.named_parameters() if q.grad is not None}
    assert sorted(got) == sorted(names), f"parameters with a gradient on the device: {sorted(set(got) ^ set(names))}"
    for k in names:
        close(got[k], leaves[PRE + k].grad, k, log, **STEP_TOL)
    report(tag, log)
