"""Host half of the post-context fusion: the feature header (include/t4r_hip_postfusion.h) and its binding through
_lib.FEATURE_HEADERS, the size query and the argument limits (refused before any launch), the float64 restatement
(tests/post_fusion_restatement.py) against the reference's own PostContextFusion built live (oracle/ref_standins.py), its bounds
against the fp32 torch chain and against planted faults, the registered operators' fakes and make_fx, the module's attribute
contract and the state-dict keys of a Model with and without fusion.  Nothing here needs a GPU."""
import ctypes
import os
import re

import pytest
import torch
from torch.fx.experimental.proxy_tensor import make_fx

import post_fusion_restatement as R
import transformers4rec_amd as tr
from transformers4rec_amd import _lib, ops, torch_ops  # noqa: F401
from transformers4rec_amd.experimental import PostContextFusion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "t4r_hip_postfusion.h"
FOUR = ["t4r_post_fusion_bwd", "t4r_post_fusion_bwd_ws_floats", "t4r_post_fusion_fwd", "t4r_post_fusion_supported"]
V, L, D = 50, 20, 64


# ---------------------------------------------------------------------------------------------------------- header and binding
def test_header_parses_and_is_bound_through_the_feature_tuple():
    assert HEADER in _lib.FEATURE_HEADERS
    assert HEADER not in _lib.HEADERS and HEADER not in _lib.EXTENSION_HEADERS
    assert "t4r_hip.h" in _lib.HEADERS and "t4r_hip_uni.h" in _lib.EXTENSION_HEADERS        # the other two tuples are as they were
    assert _lib.header_symbols(HEADER) == FOUR
    feat = _lib.feature_signatures()
    assert set(FOUR) <= set(feat)
    assert not set(feat) & set(_lib.signatures()) and not set(feat) & set(_lib.extension_signatures())
    assert feat["t4r_post_fusion_supported"] == ("i", "ii")
    assert feat["t4r_post_fusion_bwd_ws_floats"] == ("l", "liiiii")
    assert feat["t4r_post_fusion_fwd"] == ("i", "p" * 6 + "l" + "i" * 5)
    assert feat["t4r_post_fusion_bwd"] == ("i", "p" * 11 + "l" + "i" * 5)
    lib = _lib.load()
    for name in FOUR:
        fn = getattr(lib, name)
        ret, args = feat[name]
        assert fn.restype is _lib._C[ret] and list(fn.argtypes) == [_lib._C[a] for a in args], name
    text = open(_lib.header_path(HEADER)).read()
    for entry in ("int t4r_post_fusion_fwd(void* stream", "int t4r_post_fusion_bwd(void* stream"):
        decl = text[: text.index(entry)]
        comment = decl[decl.rindex("/*"):]
        assert "replaces:" in comment and "experimental.py" in comment, entry
    decls = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for word in ("at::", "torch", "Tensor", "std::", "c10"):
        assert word not in decls, f"{word} leaked into the C ABI"
    assert "t4r_hip_postfusion.h" in open(os.path.join(ROOT, "transformers4rec_amd", "build.py")).read()


def test_a_feature_name_that_repeats_another_header_is_an_error(monkeypatch):
    monkeypatch.setattr(_lib, "FEATURE_HEADERS", ("t4r_hip_uni.h",))
    _lib.feature_signatures.cache_clear()
    try:
        with pytest.raises(_lib.T4RHipError, match="already declared"):
            _lib.feature_signatures()
    finally:
        monkeypatch.undo()
        _lib.feature_signatures.cache_clear()
    assert set(FOUR) <= set(_lib.feature_signatures())


# ---------------------------------------------------------------------------------------------------------- limits
BUF = ctypes.c_void_p(1 << 20)        # never dereferenced: every failing case below is refused before any launch


def _fwd(lib, ntok=21, L=7, D=8, C=4, mode=0, ps=0, seq=BUF, W=BUF, b=BUF):
    return lib.t4r_post_fusion_fwd(None, seq, BUF, W, b, BUF, ntok, L, D, C, mode, ps)


def _bwd(lib, ntok=21, L=7, D=8, C=4, mode=0, ps=0, seq=BUF, W=BUF, b=BUF, d_w=None):
    return lib.t4r_post_fusion_bwd(None, BUF, seq, BUF, W, b, BUF, BUF, d_w, None, BUF, ntok, L, D, C, mode, ps)


def test_limits_and_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    got = [lib.t4r_post_fusion_supported(*a) for a in ((1, 1), (1024, 256), (0, 4), (1025, 4), (8, 0), (8, 257))]
    assert got == [1, 1, 0, 0, 0, 0]
    assert ops.post_fusion_supported(64, 24) and not ops.post_fusion_supported(64, 300)
    for call in (_fwd, _bwd):
        for kw, word in ((dict(D=0), b"D"), (dict(D=1025), b"D"), (dict(C=0), b"C"), (dict(C=257), b"C"), (dict(L=4), b"L"),
                         (dict(L=0), b"L"), (dict(ntok=-1), b"ntok"), (dict(ntok=1 << 31), b"ntok"), (dict(mode=3), b"mode"),
                         (dict(mode=-1), b"mode"), (dict(mode=2), b"concat"), (dict(mode=2, b=None), b"concat"),
                         (dict(seq=None), b"null"), (dict(W=None), b"null"), (dict(seq=ctypes.c_void_p((1 << 20) + 2)), b"aligned")):
            assert call(lib, **kw) != 0, (call.__name__, kw)
            assert word in lib.t4r_last_error(), (call.__name__, kw, lib.t4r_last_error())
    assert _bwd(lib, mode=2, W=None, b=None, d_w=BUF) != 0 and b"concat" in lib.t4r_last_error()
    # ntok = 0: nothing launches, nothing is looked at
    assert lib.t4r_post_fusion_fwd(None, None, None, None, None, None, 0, 7, 8, 4, 0, 0) == 0
    assert lib.t4r_post_fusion_bwd(None, None, None, None, None, None, None, None, None, None, None, 0, 7, 8, 4, 1, 1) == 0
    seq, ctx, W, b = torch.zeros(2, 3, 8), torch.zeros(2, 3, 4), torch.zeros(8, 4), torch.zeros(8)
    with pytest.raises(_lib.T4RHipError, match="GPU"):
        ops.post_fusion_fwd(seq, ctx, W, b, 0)
    with pytest.raises(_lib.T4RHipError, match="GPU"):
        ops.post_fusion_bwd_(seq, seq, ctx, W, b, 0)


def test_ws_floats_is_pure_monotone_and_zero_outside_the_limits():
    f = _lib.load().t4r_post_fusion_bwd_ws_floats
    for args in ((0, 1, 64, 24, 0, 0), (-5, 1, 64, 24, 0, 0), (1 << 31, 1, 64, 24, 0, 0), (21, 7, 0, 24, 0, 0), (21, 7, 1025, 24, 0, 0),
                 (21, 7, 64, 0, 0, 0), (21, 7, 64, 257, 0, 0), (21, 4, 64, 24, 0, 0), (21, 0, 64, 24, 0, 0), (21, 7, 64, 24, 3, 0),
                 (21, 7, 64, 24, -1, 0), (21, 7, 64, 24, 2, 0), (21, 7, 64, 24, 2, 1)):
        assert f(*args) == 0, args
    Ts = [1, 21, 63, 64, 65, 260, 1024, 20480, 100000, 3_000_000, (1 << 31) - 1]
    for Dm, C in ((1, 1), (64, 24), (100, 65), (1024, 256)):
        for mode in (0, 1):
            for ps in (0, 1):
                got = [f(T, 1, Dm, C, mode, ps) for T in Ts]
                assert got == [f(T, 1, Dm, C, mode, ps) for T in Ts] and got == sorted(got), (Dm, C, got)
                assert got[0] >= Dm * (C + 1) + ps * C
    assert f(260, 20, 64, 24, 0, 1) == f(260, 20, 64, 24, 0, 0) + 260 * 24


# ---------------------------------------------------------------------------------------------------------- against the reference
class _Last(torch.nn.Module):
    def __init__(self, L, D):
        super().__init__()
        self.L, self.D = L, D

    def output_size(self, input_size=None):
        return [-1, self.L, self.D]


class _Seq(torch.nn.Module):
    """stands for the reference's sequential module: hands on the batch's own [B, L, D] tensor"""

    def __init__(self, L, D):
        super().__init__()
        self.inputs, self.last = None, _Last(L, D)

    def __getitem__(self, i):
        return self.last

    def forward(self, inputs, training=False, testing=False, **kw):
        return inputs["seq"]


class _Ctx(torch.nn.Module):
    def __init__(self, C):
        super().__init__()
        self.C = C

    def output_size(self, input_size=None):
        return [-1, self.C]

    def forward(self, inputs, training=False, **kw):
        return inputs["ctx"]


def _reference_class():
    import ref_standins as rs

    if not os.path.isdir(rs.REFERENCE_ROOT):
        pytest.skip("the reference tree is not on this machine")
    rs.import_reference()
    from transformers4rec.torch.experimental import PostContextFusion as Ref

    return Ref


def _close64(got, want, what):
    scale = max(float(want.abs().max()), 1e-300)
    assert float((got.double() - want.double()).abs().max()) <= 1e-12 * scale, what


@pytest.mark.parametrize("mode", R.MODES)
def test_restatement_equals_the_reference_block_in_float64(mode):
    Ref = _reference_class()
    B, Ls, Dm, C = 3, 5, 8, 6
    k = R.make_case(B, Ls, Dm, C, False)
    fusion = Ref(_Seq(Ls, Dm), _Ctx(C), R.AGGREGATION[mode]).double()
    seq, ctx = k["seq"].double().requires_grad_(), k["ctx"].double().requires_grad_()
    out = fusion({"seq": seq, "ctx": ctx}, training=True)
    dout = (k["dout_cat"] if mode == "concat" else k["dout"]).double()
    out.backward(dout)
    lin = getattr(fusion, "context_projection", None)
    W = lin.weight.detach() if lin is not None else k["W"]
    b = lin.bias.detach() if lin is not None else k["b"]
    want, _ = R.forward(seq.detach(), ctx.detach(), W, b, mode)
    _close64(want, out.detach(), "out")
    g = R.gradients(dout, seq.detach(), ctx.detach(), W, b, mode)
    _close64(g["dseq"][0], seq.grad, "dseq")
    _close64(g["dctx"][0], ctx.grad, "dctx")
    if lin is not None:
        _close64(g["d_w"][0], lin.weight.grad, "d_w")
        _close64(g["d_b"][0], lin.bias.grad, "d_b")
        assert tuple(lin.weight.shape) == (Dm, C) and fusion.last_dim == Dm
    else:
        assert fusion.last_dim == Dm + C
    assert fusion.output_size() == [-1, Ls, fusion.last_dim]


def test_the_reference_raises_for_a_2d_context_and_for_an_unknown_aggregation():
    Ref = _reference_class()
    k = R.make_case(3, 5, 8, 6, True)
    with pytest.raises(AttributeError, match="sequence_length"):
        Ref(_Seq(5, 8), _Ctx(6), "elementwise-mul")({"seq": k["seq"], "ctx": k["ctx"]}, training=True)
    with pytest.raises(ValueError) as ref_err:
        Ref(_Seq(5, 8), _Ctx(6), "foo")({"seq": k["seq"], "ctx": k["ctx"][:, None].expand(-1, 5, -1)})
    with pytest.raises(ValueError) as our_err:
        PostContextFusion(*_parts()[:2], "foo")
    assert str(our_err.value) == str(ref_err.value)


# ---------------------------------------------------------------------------------------------------------- bounds and faults
SHAPES = [(3, 7, 64, 1), (5, 13, 100, 65), (13, 20, 128, 24), (4, 20, 128, 256)]


@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("session", [False, True], ids=["sequence", "session"])
@pytest.mark.parametrize("B,Ls,Dm,C", SHAPES)
def test_the_fp32_torch_chain_stays_inside_the_bounds(B, Ls, Dm, C, session, scale):
    k = R.make_case(B, Ls, Dm, C, session, scale)
    for mode in R.MODES:
        out, grads = R.torch_chain(k, mode, accumulate=True)
        want, bound = R.forward(k["seq"], k["ctx"], k["W"], k["b"], mode)
        assert R.ratio(out, want, bound) <= 1.0, (mode, "out")
        dout = k["dout_cat"] if mode == "concat" else k["dout"]
        ref = R.gradients(dout, k["seq"], k["ctx"], k["W"], k["b"], mode, k["d_w0"], k["d_b0"])
        for name, (val, bnd) in ref.items():
            assert R.ratio(grads[name], val, bnd) <= 1.0, (mode, name, R.ratio(grads[name], val, bnd))


def test_planted_faults_exceed_their_bounds():
    k = R.make_case(5, 13, 100, 65, True)
    for mode, faults in (("mul", ("no_one_plus", "no_bias", "c_truncated", "session_row_mod")),
                         ("sum", ("no_bias", "c_truncated", "session_row_mod"))):
        want, bound = R.forward(k["seq"], k["ctx"], k["W"], k["b"], mode)
        for fault in faults:
            bad, _ = R.forward(k["seq"], k["ctx"], k["W"], k["b"], mode, fault=fault)
            assert R.ratio(bad.float(), want, bound) > 10.0, (mode, fault)
    cases = (("mul", "dw_overwritten", "d_w", k["dout"]), ("sum", "dw_overwritten", "d_w", k["dout"]),
             ("mul", "dctx_last_token", "dctx", k["dout"]), ("sum", "dctx_last_token", "dctx", k["dout"]),
             ("concat", "dctx_last_token", "dctx", k["dout_cat"]), ("mul", "g_of_sum", "d_w", k["dout"]),
             ("mul", "g_of_sum", "d_b", k["dout"]), ("mul", "g_of_sum", "dctx", k["dout"]))
    for mode, fault, name, dout in cases:
        good = R.gradients(dout, k["seq"], k["ctx"], k["W"], k["b"], mode, k["d_w0"], k["d_b0"])
        bad = R.gradients(dout, k["seq"], k["ctx"], k["W"], k["b"], mode, k["d_w0"], k["d_b0"], fault=fault)
        assert R.ratio(bad[name][0].float(), *good[name]) > 10.0, (mode, fault, name)
    assert set(R.FAULTS) == {"no_one_plus", "no_bias", "c_truncated", "session_row_mod", "dw_overwritten", "dctx_last_token", "g_of_sum"}


# ---------------------------------------------------------------------------------------------------------- operators
def test_operators_are_registered_and_their_fakes_give_the_shapes():
    assert {"post_fusion", "post_fusion_bwd"} <= set(torch_ops.OPERATORS)
    for name in ("post_fusion", "post_fusion_bwd"):
        assert str(getattr(torch.ops.t4r_hip, name).default._schema).startswith(f"t4r_hip::{name}(")
    m = lambda *s: torch.empty(*s, device="meta")     # noqa: E731
    assert torch.ops.t4r_hip.post_fusion(m(5, 7, 64), m(5, 7, 24), m(64, 24), m(64), 0).shape == (5, 7, 64)
    assert torch.ops.t4r_hip.post_fusion(m(5, 7, 64), m(5, 24), m(64, 24), m(64), 1).shape == (5, 7, 64)
    assert torch.ops.t4r_hip.post_fusion(m(5, 7, 64), m(5, 24), None, None, 2).shape == (5, 7, 88)
    g = torch.ops.t4r_hip.post_fusion_bwd(m(5, 7, 64), m(5, 7, 64), m(5, 24), m(64, 24), m(64), 0)
    assert [tuple(t.shape) for t in g] == [(5, 7, 64), (5, 24), (64, 24), (64,)]
    g = torch.ops.t4r_hip.post_fusion_bwd(m(5, 7, 88), m(5, 7, 64), m(5, 7, 24), None, None, 2)
    assert [tuple(t.shape) for t in g] == [(5, 7, 64), (5, 7, 24), (0,), (0,)]


def test_make_fx_traces_the_operator_and_its_backward_on_meta_tensors():
    def f(seq, ctx, W, b):
        out = torch.ops.t4r_hip.post_fusion(seq, ctx, W, b, 0)
        return torch.autograd.grad(out.sum(), (seq, ctx, W, b))

    m = lambda *s: torch.empty(*s, device="meta", requires_grad=True)     # noqa: E731
    gm = make_fx(f, tracing_mode="fake")(m(5, 7, 64), m(5, 24), m(64, 24), m(64))
    targets = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
    assert "t4r_hip.post_fusion.default" in targets and "t4r_hip.post_fusion_bwd.default" in targets, targets


# ---------------------------------------------------------------------------------------------------------- module
def _parts(context="session", masking="clm"):
    torch.manual_seed(0)
    feats = tr.TabularSequenceFeatures.from_schema(tr.session_schema(V, L), max_sequence_length=L, masking=masking,
                                                   aggregation="concat", embedding_dims={"item_id": D})
    cfg = tr.XLNetConfig.build(d_model=D, n_head=4, n_layer=2, total_seq_length=L, dropout=0.0)
    block = tr.TransformerBlock(cfg, masking=feats.masking)
    if context == "session":
        ctx = tr.EmbeddingFeatures({"user": tr.FeatureConfig(tr.TableConfig(11, 8, name="user")),
                                    "country": tr.FeatureConfig(tr.TableConfig(7, 16, name="country"))}, aggregation="concat")
    else:
        ctx = tr.SequenceEmbeddingFeatures({"category": (13, 24)}, aggregation="concat")
    return feats, block, ctx


@pytest.mark.parametrize("aggregation", ["elementwise-mul", "elementwise-sum", "concat"])
def test_module_attributes_follow_the_reference_contract(aggregation):
    feats, block, ctx = _parts()
    f = PostContextFusion((feats, block), ctx, aggregation)
    assert tr.experimental.PostContextFusion is PostContextFusion
    assert f.sequential_module[0] is feats and f.sequential_module[1] is block and f.post_context_module is ctx
    assert f.fusion_aggregation == aggregation and f.inputs is feats and f.seq_length == L
    assert f._get_name() == "PostContextFusion"
    if aggregation == "concat":
        assert f.last_dim == D + 24 and not hasattr(f, "context_projection")
    else:
        lin = f.context_projection
        assert f.last_dim == D and tuple(lin.weight.shape) == (D, 24) and tuple(lin.bias.shape) == (D,)
        bound = 1 / 24 ** 0.5                                   # torch.nn.Linear's default init
        assert 0 < float(lin.weight.detach().abs().max()) <= bound and float(lin.bias.detach().abs().max()) <= bound
    assert f.output_size() == [-1, L, f.last_dim]
    assert f.forward_output_size(torch.Size([8, L, D])) == torch.Size([8, L, f.last_dim])
    names = {n for n, _ in f.named_parameters()}
    assert {id(p) for p in tr.hip_parameters(f)} == {id(p) for p in f.parameters()}
    assert "post_context_module.embedding_tables.user.weight" in names
    with pytest.raises(_lib.T4RHipError, match="GPU"):
        f.fuse(torch.zeros(2, L, D), torch.zeros(2, 24))


def test_limits_of_the_module():
    feats, block, _ = _parts()
    wide = tr.EmbeddingFeatures({"user": tr.FeatureConfig(tr.TableConfig(11, 257, name="user"))}, aggregation="concat")
    with pytest.raises(ValueError, match="C <= 256"):
        PostContextFusion((feats, block), wide)
    with pytest.raises(ValueError, match="output_size"):
        PostContextFusion((feats, block), tr.EmbeddingFeatures({"user": tr.FeatureConfig(tr.TableConfig(11, 8, name="user"))}))
    with pytest.raises(ValueError, match="aggregation='concat'"):          # a dict of sizes: the context is not concatenated
        PostContextFusion((feats, block), tr.SequenceEmbeddingFeatures({"a": (5, 6)}))
    seq_ctx = tr.SequenceEmbeddingFeatures({"b": (5, 4), "a": (5, 6)}, aggregation="concat")
    assert seq_ctx.output_size() == torch.Size([-1, -1, 10]) and tr.SequenceEmbeddingFeatures({"a": (5, 6)}).aggregation is None
    with pytest.raises(NotImplementedError):
        tr.SequenceEmbeddingFeatures({"a": (5, 6)}, aggregation="sum")


def _keys(model):
    return {k: tuple(v.shape) for k, v in model.state_dict().items()}


@pytest.mark.parametrize("context", ["session", "sequence"])
def test_state_dict_keys_of_a_model_with_and_without_fusion(context):
    feats, block, _ = _parts()
    plain = tr.Model(feats, block, tr.NextItemPredictionTask(weight_tying=True))
    assert plain.input_features is feats and plain.transformer_block is block
    assert type(plain.heads[0].body).__name__ == "_Body"
    plain_keys = _keys(plain)
    assert all(k.startswith(("heads.0.body.0.", "heads.0.body.1.", "heads.0.prediction_task_dict.next-item.")) for k in plain_keys)
    for aggregation in ("elementwise-mul", "concat"):
        feats, block, ctx = _parts(context)
        fused = tr.Model(feats, block, tr.NextItemPredictionTask(weight_tying=True), post_context_module=ctx,
                         fusion_aggregation=aggregation)
        body = fused.heads[0].body
        assert isinstance(body, PostContextFusion) and fused.input_features is feats and fused.transformer_block is block
        keys = _keys(fused)
        C = 24
        moved = {k.replace("heads.0.body.", "heads.0.body.sequential_module.", 1) if k.startswith("heads.0.body.") else k: v
                 for k, v in plain_keys.items()}
        extra = {k: v for k, v in keys.items() if k not in moved}
        table = ({"heads.0.body.post_context_module.embedding_tables.user.weight": (11, 8),
                  "heads.0.body.post_context_module.embedding_tables.country.weight": (7, 16)} if context == "session"
                 else {"heads.0.body.post_context_module.embedding_tables.category.weight": (13, 24)})
        if aggregation == "concat":
            # the tied head's projection Linear(D + C, item_dim) takes the wider input
            proj = {k: v for k, v in extra.items() if "task_block" in k}
            assert sorted(proj.values()) == [(D,), (D, D + C)], proj
            assert {k: v for k, v in extra.items() if k not in proj} == table
        else:
            assert extra == dict(table, **{"heads.0.body.context_projection.weight": (D, C), "heads.0.body.context_projection.bias": (D,)})
        assert set(moved) <= set(keys)
        from transformers4rec_amd.model import last_rows_gate
        assert last_rows_gate(fused, True, 8, L, n_labels=1) is None


# ---------------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name,aggregation", [("post_fusion_mul_train", "elementwise-mul"), ("post_fusion_sum_train", "elementwise-sum"),
                                              ("post_fusion_concat_train", "concat")])
def test_fixture_parameters_have_a_home_in_the_mirror_and_hold_data_only(name, aggregation):
    import golden_utils as gu

    d = gu.load(name)
    assert os.path.getsize(os.path.join(gu.GOLDEN, name + ".npz")) <= 900 * 1024
    assert str(d["meta/fusion_aggregation"]) == aggregation
    assert all(v.dtype.kind in "fiubU" for v in d.values())                 # arrays of numbers and meta strings, nothing else
    feats = tr.TabularSequenceFeatures.from_schema(tr.session_schema(int(d["meta/V"]) - 1, int(d["meta/L"])), max_sequence_length=int(d["meta/L"]),
                                                   masking="clm", aggregation="concat", embedding_dims={"item_id": int(d["meta/d_item"])})
    cfg = tr.XLNetConfig.build(d_model=int(d["meta/d_model"]), n_head=int(d["meta/n_head"]), n_layer=int(d["meta/n_layer"]),
                               total_seq_length=int(d["meta/L"]), dropout=0.0)
    ctx = tr.SequenceEmbeddingFeatures({"category": (int(d["meta/cat_card"]) + 1, int(d["meta/cat_dim"]))}, aggregation="concat")
    model = tr.Model(feats, tr.TransformerBlock(cfg, masking=feats.masking), tr.NextItemPredictionTask(weight_tying=True),
                     post_context_module=ctx, fusion_aggregation=aggregation)
    own = _keys(model)
    ref = {k: tuple(v.shape) for k, v in gu.section(d, "p/").items()}
    assert ref and all(own.get(k) == v for k, v in ref.items()), [k for k, v in ref.items() if own.get(k) != v]
    assert "heads.0.body.post_context_module.embedding_tables.category.weight" in ref
    assert ("heads.0.body.context_projection.weight" in ref) == (aggregation != "concat")
    grads = gu.section(d, "g/")
    assert set(grads) <= set(dict(model.named_parameters())) and len(grads) >= 20
