"""XLNet attn_type='uni' without a GPU: the restatement of tests/xlnet_uni_restatement.py against the installed HF
XLNetModel(attn_type='uni'), its causality, the configuration, the extension-header binding, the registered operator and the
drop-in boundary."""
import ctypes
import types

import pytest
import torch

import attn_core_restatement as R
import t4r_oracle as O
import xlnet_uni_restatement as U

F64 = torch.float64


def _hf_model(transformers, D, n, layers, attn_type="uni", seed=0):
    cfg = transformers.XLNetConfig(
        d_model=D, d_inner=4 * D, n_layer=layers, n_head=n, attn_type=attn_type, ff_activation="gelu",
        initializer_range=0.01, layer_norm_eps=0.03, dropout=0.0, pad_token_id=0, vocab_size=1, mem_len=1)
    torch.manual_seed(seed)
    m = transformers.XLNetModel(cfg).eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            p.copy_(1 + 0.1 * torch.randn_like(p) if "layer_norm.weight" in name else 0.1 * torch.randn_like(p))
    return m


# ------------------------------------------------------------------------------------------------ restatement against HF
@pytest.mark.parametrize("B,L,D,n,layers", [(3, 1, 32, 2, 1), (2, 7, 32, 4, 2), (2, 20, 64, 4, 2)])
def test_uni_restatement_matches_hf(B, L, D, n, layers):
    transformers = pytest.importorskip("transformers")
    m = _hf_model(transformers, D, n, layers)
    x = torch.randn(B, L, D, requires_grad=True)
    ref = m(inputs_embeds=x)[0]
    xo = x.detach().clone().requires_grad_()
    lp = [{k: v.detach().clone().requires_grad_() for k, v in O.xlnet_layer_params_from_hf(l).items()} for l in m.layer]
    got = U.model(xo, lp, n, 0.03, causal=True)
    torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-5)
    w = torch.randn(B, L, D)
    (ref * w).sum().backward()
    (got * w).sum().backward()
    torch.testing.assert_close(xo.grad, x.grad, rtol=1e-4, atol=2e-5)
    hf_names = dict(q="rel_attn.q", k="rel_attn.k", v="rel_attn.v", o="rel_attn.o", r="rel_attn.r", r_w_bias="rel_attn.r_w_bias",
                    r_r_bias="rel_attn.r_r_bias", ln_w="rel_attn.layer_norm.weight", ln_b="rel_attn.layer_norm.bias",
                    w1="ff.layer_1.weight", b1="ff.layer_1.bias", w2="ff.layer_2.weight", b2="ff.layer_2.bias",
                    ff_ln_w="ff.layer_norm.weight", ff_ln_b="ff.layer_norm.bias")
    for li, layer in enumerate(m.layer):
        hf = dict(layer.named_parameters())
        for ours, theirs in hf_names.items():
            torch.testing.assert_close(lp[li][ours].grad, hf[theirs].grad, rtol=1e-4, atol=2e-5, msg=lambda s, o=ours: f"{o}: {s}")
    if L > 1:       # and the causal flag matters on these inputs
        assert float((got - U.model(xo, lp, n, 0.03, causal=False)).detach().abs().max()) > 1e-3


def test_bi_flag_of_the_restatement_is_the_oracle():
    g = torch.Generator().manual_seed(3)
    B, L, D, n = 2, 9, 32, 2
    p = U.layer_params(g, D, n, dtype=F64)
    x = torch.randn(B, L, D, generator=g, dtype=F64)
    kl = torch.tensor([4, 9], dtype=torch.int32)
    torch.testing.assert_close(U.layer(x, p, n), O.xlnet_layer(x, p, n), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(U.layer(x, p, n, key_len=kl), O.xlnet_layer(x, p, n, key_len=kl), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------ causality
@pytest.mark.parametrize("t", [0, 3, 8])
def test_restated_model_is_causal(t):
    g = torch.Generator().manual_seed(5)
    B, L, D, n = 2, 10, 32, 2
    lp = [U.layer_params(g, D, n, dtype=F64) for _ in range(2)]
    x = torch.randn(B, L, D, generator=g, dtype=F64)
    y = x.clone()
    y[:, t + 1:] = torch.randn(B, L - t - 1, D, generator=g, dtype=F64)
    a, b = U.model(x, lp, n, causal=True), U.model(y, lp, n, causal=True)
    assert torch.equal(a[:, :t + 1], b[:, :t + 1])
    assert not torch.equal(a[:, t + 1:], b[:, t + 1:])
    a, b = U.model(x, lp, n, causal=False), U.model(y, lp, n, causal=False)
    assert not torch.equal(a[:, :t + 1], b[:, :t + 1])          # the bi body leaks: the comparison can see it


def test_restated_core_dead_pairs_and_relative_rows():
    """the float64 core: p = 0 with a zero bound at every dead pair; rows 0 and L + 1 .. 2L - 1 of dkr exactly zero, their
    bound nothing but the format's underflow terms (2^-126 per pair, attn_core_restatement: e_dS)"""
    B, L, n, d = 5, 7, 2, 4
    x = R.family("U", B, L, n, d, 0)
    kl = R.mask_edges(L)
    for key_len in (None, kl):
        ref = U.reference(x, key_len=key_len)
        bd = U.bounds(x, ref, key_len=key_len)
        dead = U.uni_dead(B, L, key_len).expand(B, n, L, L)
        assert bool((ref["prob"][dead] == 0).all()) and bool((bd["prob"][dead] == 0).all())
        assert torch.allclose(ref["prob"].sum(3), torch.ones(B, n, L, dtype=F64))
        for rows in (slice(0, 1), slice(L + 1, 2 * L)):
            assert float(ref["dkr"][rows].abs().max()) == 0.0 and float(bd["dkr"][rows].max()) < 1e-30
        assert float(ref["dkr"][1:L + 1].abs().min()) > 0.0
    assert R.xlnet_dead is U.R_XLNET_DEAD                        # the substitution lasts for the call only
    # key_len = 0: every row attends to itself alone, as in the bi core
    assert torch.equal(U.reference(x, key_len=kl)["prob"][0], torch.eye(L, dtype=F64).expand(n, L, L))


def test_training_mode_restatement_with_all_ones_masks_is_the_eval_form():
    g = torch.Generator().manual_seed(6)
    B, L, D, n = 2, 6, 32, 2
    lp = [U.layer_params(g, D, n, dtype=F64) for _ in range(2)]
    x = torch.randn(B, L, D, generator=g, dtype=F64)
    one = lambda *s: torch.ones(*s, dtype=torch.uint8)
    masks = dict(input=one(B, L, D), pos=one(B, 2 * L, D), final=one(B, L, D),
                 layers=[dict(prob=one(B, n, L, L), attn_out=one(B, L, D), ff_act=one(B, L, 4 * D), ff_out=one(B, L, D))] * 2)
    torch.testing.assert_close(U.model(x, lp, n, causal=True, masks=masks, drop_p=0.0), U.model(x, lp, n, causal=True),
                               rtol=1e-12, atol=1e-12)
    dm = U.device_masks(B, L, D, n, 2, 0.3, 11, 1)
    assert dm["pos"].shape == (B, 2 * L, D) and dm["layers"][1]["prob"].shape == (B, n, L, L)
    lm = U.layer_device_masks(B, L, D, n, 0.3, 11, 1, 1)
    assert torch.equal(lm["prob"], dm["layers"][1]["prob"]) and torch.equal(lm["pos"], dm["pos"])
    got = U.model(x, lp, n, causal=True, masks=dm, drop_p=0.3)
    assert bool(torch.isfinite(got).all()) and float((got - U.model(x, lp, n, causal=True)).abs().max()) > 1e-2


# ------------------------------------------------------------------------------------------------ configuration
def test_config_accepts_bi_and_uni_only():
    import transformers4rec_amd as tr

    cfg = tr.XLNetConfig.build(32, 2, 2, total_seq_length=20, attn_type="uni")
    assert isinstance(cfg, tr.XLNetConfig) and cfg.attn_type == "uni"
    assert tr.XLNetConfig.build(32, 2, 2, total_seq_length=20).attn_type == "bi"
    with pytest.raises(ValueError, match="'bi'.*'uni'"):
        tr.XLNetConfig.build(32, 2, 2, total_seq_length=20, attn_type="x")


def test_transformer_block_accepts_both_maskings_for_uni():
    import transformers4rec_amd as tr
    from transformers4rec_amd.masking import CausalLanguageModeling, MaskedLanguageModeling

    cfg = tr.XLNetConfig.build(32, 2, 1, total_seq_length=20, attn_type="uni")
    for masking in (CausalLanguageModeling(32), MaskedLanguageModeling(32), None):
        for mask_padding in (False, True):
            blk = tr.TransformerBlock(cfg, masking=masking, mask_padding=mask_padding)
            assert blk.transformer.config.attn_type == "uni"


def test_functional_step_refuses_uni():
    import transformers4rec_amd as tr
    from transformers4rec_amd import functional

    L, D = 20, 32
    schema = tr.session_schema(99, L)
    inputs = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking="mlm", embedding_dim_default=D)
    cfg = tr.XLNetConfig.build(D, 2, 1, total_seq_length=L, attn_type="uni")
    model = cfg.to_torch_model(inputs, tr.NextItemPredictionTask(weight_tying=True))
    with pytest.raises(NotImplementedError, match="uni"):
        functional.config_of(model)


# ------------------------------------------------------------------------------------------------ binding
UNI_NAMES = ["t4r_xlnet_attn_uni_bwd", "t4r_xlnet_attn_uni_fwd", "t4r_xlnet_layer_uni_bwd", "t4r_xlnet_layer_uni_fwd"]
CTYPES = {"p": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_long, "f": ctypes.c_float, "Q": ctypes.c_ulonglong,
          "s": ctypes.c_char_p, "v": None}


def test_extension_header_is_bound_beside_the_main_headers():
    from transformers4rec_amd import _lib

    assert "t4r_hip_uni.h" not in _lib.HEADERS and len(_lib.HEADERS) == 12 and len(_lib.signatures()) == 170
    assert _lib.EXTENSION_HEADERS == ("t4r_hip_uni.h",)
    ext = _lib.extension_signatures()
    assert sorted(ext) == UNI_NAMES == _lib.header_symbols("t4r_hip_uni.h")
    assert not set(ext) & set(_lib.signatures())
    assert not set(_lib.header_symbols()) & set(ext)
    main = _lib.signatures()
    for bi, uni in (("t4r_xlnet_attn_fwd", "t4r_xlnet_attn_uni_fwd"), ("t4r_xlnet_attn_bwd", "t4r_xlnet_attn_uni_bwd"),
                    ("t4r_xlnet_layer_fwd", "t4r_xlnet_layer_uni_fwd"), ("t4r_xlnet_layer_bwd", "t4r_xlnet_layer_uni_bwd")):
        assert ext[uni] == main[bi], uni                         # the parameters of the bi entries
    lib = _lib.load()
    for name, (ret, args) in ext.items():
        assert hasattr(lib, name), f"{name} is declared in t4r_hip_uni.h but not exported"
        fn = getattr(lib, name)
        assert fn.restype is CTYPES[ret] and list(fn.argtypes) == [CTYPES[a] for a in args], name


def test_a_name_of_the_main_headers_in_an_extension_header_is_an_error(monkeypatch, tmp_path):
    from transformers4rec_amd import _lib

    (tmp_path / "a.h").write_text("int f(int a);\n")
    (tmp_path / "e.h").write_text("long g(long n);\nint f(int a);\n")
    monkeypatch.setattr(_lib, "header_path", lambda name: str(tmp_path / name))
    monkeypatch.setattr(_lib, "HEADERS", ("a.h",))
    monkeypatch.setattr(_lib, "EXTENSION_HEADERS", ("e.h",))
    try:
        _lib.signatures.cache_clear()
        _lib.extension_signatures.cache_clear()
        with pytest.raises(_lib.T4RHipError, match="`f`.*e.h"):
            _lib.extension_signatures()
    finally:
        _lib.signatures.cache_clear()
        _lib.extension_signatures.cache_clear()
        _lib._header_signatures.cache_clear()


def test_argument_errors_come_back_before_any_launch():
    from transformers4rec_amd import _lib

    lib = _lib.load()
    rc = lib.t4r_xlnet_attn_uni_fwd(None, None, None, None, None, None, None, None, None, 1, 20, 4, 300, 0, 0.0, 0, 0, None)
    assert rc != 0 and b"d_head" in lib.t4r_last_error()
    rc = lib.t4r_xlnet_attn_uni_fwd(None, None, None, None, None, None, None, None, None, 1, 20, 4, 16, 0, 0.0, 0, 0, None)
    assert rc != 0 and b"null" in lib.t4r_last_error()
    assert lib.t4r_xlnet_attn_uni_fwd(None, None, None, None, None, None, None, None, None, 0, 20, 4, 16, 0, 0.0, 0, 0, None) == 0


# ------------------------------------------------------------------------------------------------ operator
def test_operator_is_registered_and_propagates_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from transformers4rec_amd import torch_ops

    assert "xlnet_layer_uni_infer" in torch_ops.OPERATORS
    assert str(torch.ops.t4r_hip.xlnet_layer_uni_infer.default._schema).startswith("t4r_hip::xlnet_layer_uni_infer(")
    B, L, D, n = 3, 20, 64, 4
    with FakeTensorMode():
        g = torch.Generator().manual_seed(0)
        prm = [torch.empty(*v.shape, device="cuda") for v in U.layer_params(g, D, n).values()]
        h, pos = torch.empty(B * L, D, device="cuda"), torch.empty(2 * L, D, device="cuda")
        out = torch.ops.t4r_hip.xlnet_layer_uni_infer(h, pos, prm, B, L, n, 0.03, None)
        assert out.shape == (B * L, D) and out.device.type == "cuda"


def test_uni_inference_body_traces_into_uni_nodes():
    """make_fx over a TransformerBlock built with attn_type='uni' (eval, no_grad, fake tensors): one
    t4r_hip.xlnet_layer_uni_infer node per layer, none of the bi operator, nothing falls out of the trace"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.proxy_tensor import make_fx

    import transformers4rec_amd as tr

    with FakeTensorMode(), torch.device("cuda"):
        cfg = tr.XLNetConfig.build(64, 4, 2, total_seq_length=20, dropout=0.0, attn_type="uni")
        block = tr.TransformerBlock(cfg).eval()
        x = torch.empty(3, 20, 64, device="cuda")

        def f(inputs_embeds):
            with torch.no_grad():
                return block(inputs_embeds)

        gm = make_fx(f, tracing_mode="real")(x)
    targets = [str(nd.target) for nd in gm.graph.nodes if nd.op == "call_function"]
    assert sum("t4r_hip.xlnet_layer_uni_infer" in t for t in targets) == cfg.n_layer, targets
    assert not any("t4r_hip.xlnet_layer_infer" in t or "aten.mm" in t or "aten.bmm" in t or "layer_norm" in t for t in targets), targets


# ------------------------------------------------------------------------------------------------ drop-in
def test_dropin_accepts_a_reference_xlnet_built_with_uni():
    """structurally, as tests/test_dropin_cpu.py does for bi: the shadow block of an HF XLNetModel(attn_type='uni') carries
    the attention type and shares every parameter; bi_data, clamp_len and same_length stay refused"""
    transformers = pytest.importorskip("transformers")
    from transformers4rec_amd import dropin

    m = _hf_model(transformers, 32, 2, 2)
    sh = dropin.shadow_block(types.SimpleNamespace(transformer=m))
    assert sh.transformer.config.attn_type == "uni" and sh.transformer.config.hidden_size == 32
    ref_ids = {id(p) for p in m.parameters()}
    ps = dict(sh.named_parameters())
    assert ps and all(id(p) in ref_ids and p.device.type != "meta" for p in ps.values())
    assert sh.transformer.layer[1].rel_attn.r is m.layer[1].rel_attn.r
    assert dropin.shadow_block(types.SimpleNamespace(transformer=_hf_model(transformers, 32, 2, 1, "bi"))).transformer.config.attn_type == "bi"
    for field, value in (("bi_data", True), ("clamp_len", 5), ("same_length", True)):
        bad = _hf_model(transformers, 32, 2, 1)
        setattr(bad.config, field, value)
        with pytest.raises(NotImplementedError, match=field):
            dropin.shadow_block(types.SimpleNamespace(transformer=bad))
