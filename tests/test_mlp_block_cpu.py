"""Host half of the MLP block: the feature header (include/t4r_hip_mlpblock.h) and its binding through _lib.FEATURE_HEADERS, the
size query and the argument limits (refused before any launch), the float64 restatement (tests/mlp_block_restatement.py) against
the fp32 torch chain and against planted faults at the GPU test's shapes, the registered operators' fakes and make_fx, the
constructor's refusals, the module's names and initialisation, the state-dict keys of a Model with the block against the
reference's (where its tree is present) and of a Model without it against a committed fixture.  Nothing here needs a GPU."""
import ctypes
import os
import re

import pytest
import torch
from torch.fx.experimental.proxy_tensor import make_fx

import mlp_block_restatement as R
import transformers4rec_amd as tr
from transformers4rec_amd import _lib, ops, torch_ops  # noqa: F401
from transformers4rec_amd.block import DenseBlock, MLPBlock, MLPStack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "t4r_hip_mlpblock.h"
FOUR = ["t4r_mlp_stack_bwd", "t4r_mlp_stack_bwd_ws_floats", "t4r_mlp_stack_fwd", "t4r_mlp_stack_supported"]
V, L = 50, 20
SEED, OFFSET = 0x5EED1234ABCD, 3


def _ints(vals):
    return (ctypes.c_int * len(vals))(*vals)


# ---------------------------------------------------------------------------------------------------------- header and binding
def test_header_parses_and_is_bound_through_the_feature_tuple():
    assert _lib.FEATURE_HEADERS[-1] == HEADER and "t4r_hip_postfusion.h" in _lib.FEATURE_HEADERS
    assert HEADER not in _lib.HEADERS and HEADER not in _lib.EXTENSION_HEADERS
    # the other two tuples are as they were
    assert _lib.HEADERS == ("t4r_hip.h", "t4r_hip_sampling.h", "t4r_hip_filter.h", "t4r_hip_optim.h", "t4r_hip_pretrained.h",
                            "t4r_hip_attn.h", "t4r_hip_rows.h", "t4r_hip_rowadam.h", "t4r_hip_contproj.h", "t4r_hip_rowclip.h",
                            "t4r_hip_seqtask.h", "t4r_hip_rtd.h")
    assert _lib.EXTENSION_HEADERS == ("t4r_hip_uni.h",)
    assert _lib.header_symbols(HEADER) == FOUR
    feat = _lib.feature_signatures()
    assert set(FOUR) <= set(feat)
    assert not set(feat) & set(_lib.signatures()) and not set(feat) & set(_lib.extension_signatures())
    assert feat["t4r_mlp_stack_supported"] == ("i", "iip")
    assert feat["t4r_mlp_stack_bwd_ws_floats"] == ("l", "liip")
    assert feat["t4r_mlp_stack_fwd"] == ("i", "pppppp" + "l" + "iip" + "i" + "f" + "QQ")
    assert feat["t4r_mlp_stack_bwd"] == ("i", "p" * 9 + "l" + "iip" + "i" + "f" + "QQ")
    lib = _lib.load()
    for name in FOUR:
        fn = getattr(lib, name)
        ret, args = feat[name]
        assert fn.restype is _lib._C[ret] and list(fn.argtypes) == [_lib._C[a] for a in args], name
    text = open(_lib.header_path(HEADER)).read()
    for entry in ("int t4r_mlp_stack_fwd(void* stream", "int t4r_mlp_stack_bwd(void* stream"):
        decl = text[: text.index(entry)]
        comment = decl[decl.rindex("/*"):]
        assert "replaces:" in comment and "block/mlp.py" in comment and "launch" in comment, entry
    decls = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for word in ("at::", "torch", "Tensor", "std::", "c10"):
        assert word not in decls, f"{word} leaked into the C ABI"
    build = open(os.path.join(ROOT, "transformers4rec_amd", "build.py")).read()
    assert HEADER in build and '"mlp_block.hip"' in build
    assert ops.SITE_MLP_BLOCK == R.SITE == 8 and ops.SITE_MLP_BLOCK not in (ops.SITE_INPUT, ops.SITE_POS, ops.SITE_PROB,
                                                                          ops.SITE_ATTN_OUT, ops.SITE_FF_ACT, ops.SITE_FF_OUT,
                                                                          ops.SITE_FINAL, ops.SITE_GUMBEL)


# ---------------------------------------------------------------------------------------------------------- limits
BUF = ctypes.c_void_p(1 << 20)        # never dereferenced: every failing case below is refused before any launch


def _ptrs(n, p=BUF):
    return (ctypes.c_void_p * n)(*([p.value] * n))


def _fwd(lib, ntok=21, n=2, K0=8, N=(12, 4), relu=1, p=0.0, x=BUF, W="ok", acts=None, out=BUF):
    Wp = _ptrs(n) if W == "ok" else W
    return lib.t4r_mlp_stack_fwd(None, x, Wp, None, acts, out, ntok, n, K0, _ints(N) if N is not None else None, relu, p, 1, 2)


def _bwd(lib, ntok=21, n=2, K0=8, N=(12, 4), relu=1, p=0.0, dout=BUF, W="ok", acts="ok", ws=BUF, dW=None, x=BUF):
    Wp = _ptrs(n) if W == "ok" else W
    Ap = _ptrs(n) if acts == "ok" else acts
    return lib.t4r_mlp_stack_bwd(None, dout, x, Wp, Ap, BUF, dW, None, ws, ntok, n, K0, _ints(N) if N is not None else None,
                                 relu, p, 1, 2)


def test_supported_agrees_with_the_documented_limits():
    lib = _lib.load()
    cases = [((1, 1, [1]), 1), ((4, 1024, [512, 512, 512, 512]), 1), ((1, 1024, [512]), 1), ((2, 48, [96, 64]), 1),
             ((0, 8, [4]), 0), ((5, 8, [4, 4, 4, 4, 4]), 0), ((1, 0, [4]), 0), ((1, 1025, [4]), 0), ((1, 8, [0]), 0),
             ((1, 8, [513]), 0), ((3, 8, [4, 513, 4]), 0), ((2, 8, [4, -1]), 0)]
    for (n, K0, N), want in cases:
        assert lib.t4r_mlp_stack_supported(n, K0, _ints(N)) == want, (n, K0, N)
        assert ops.mlp_stack_supported(K0, N[:n]) == bool(want) or n != len(N)
    assert lib.t4r_mlp_stack_supported(1, 8, None) == 0
    assert ops.mlp_stack_supported(336, [128]) and not ops.mlp_stack_supported(336, []) and not ops.mlp_stack_supported(8, [600])
    assert (ops.MLP_MAX_LAYERS, ops.MLP_MAX_K0, ops.MLP_MAX_N) == (4, 1024, 512)


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    for call in (_fwd, _bwd):
        for kw, word in ((dict(n=0), b"layers"), (dict(n=5, N=(4, 4, 4, 4, 4)), b"layers"), (dict(K0=0), b"K0"), (dict(K0=1025), b"K0"),
                         (dict(N=(0, 4)), b"N[i]"), (dict(N=(12, 513)), b"N[i]"), (dict(N=None), b"null"), (dict(ntok=-1), b"ntok"),
                         (dict(ntok=1 << 31), b"ntok"), (dict(relu=2), b"relu"), (dict(p=1.0), b"drop_p"), (dict(p=-0.1), b"drop_p"),
                         (dict(W=None), b"null"), (dict(W=_ptrs(2, ctypes.c_void_p(0))), b"null"),
                         (dict(W=_ptrs(2, ctypes.c_void_p((1 << 20) + 2))), b"aligned")):
            assert call(lib, **kw) != 0, (call.__name__, kw)
            assert word in lib.t4r_last_error(), (call.__name__, kw, lib.t4r_last_error())
    assert _fwd(lib, x=None) != 0 and b"null" in lib.t4r_last_error()
    assert _fwd(lib, out=None) != 0 and b"null" in lib.t4r_last_error()                      # inference needs out
    assert _fwd(lib, x=ctypes.c_void_p((1 << 20) + 1)) != 0 and b"aligned" in lib.t4r_last_error()
    assert _fwd(lib, acts=_ptrs(2), out=ctypes.c_void_p(1 << 21)) != 0 and b"acts[n - 1]" in lib.t4r_last_error()
    assert _bwd(lib, dout=None) != 0 and b"null" in lib.t4r_last_error()
    assert _bwd(lib, acts=None) != 0 and b"ReLU" in lib.t4r_last_error()                     # the gate reads a_i
    assert _bwd(lib, dW=_ptrs(2), x=None) != 0 and b"input of a layer" in lib.t4r_last_error()
    assert _bwd(lib, dW=_ptrs(2), ws=None) != 0 and b"ws" in lib.t4r_last_error()
    # ntok = 0: nothing launches, nothing is looked at but the sizes
    assert lib.t4r_mlp_stack_fwd(None, None, None, None, None, None, 0, 2, 8, _ints((12, 4)), 1, 0.0, 0, 0) == 0
    assert lib.t4r_mlp_stack_bwd(None, None, None, None, None, None, None, None, None, 0, 2, 8, _ints((12, 4)), 1, 0.3, 0, 0) == 0
    x, Ws = torch.zeros(6, 8), [torch.zeros(12, 8), torch.zeros(4, 12)]
    with pytest.raises(_lib.T4RHipError, match="GPU"):
        ops.mlp_stack_fwd(x, Ws)
    with pytest.raises(_lib.T4RHipError, match="GPU"):
        ops.mlp_stack_bwd_(torch.zeros(6, 4), x, Ws, [None, None])


def test_ws_floats_is_pure_monotone_and_zero_outside_the_limits():
    f = _lib.load().t4r_mlp_stack_bwd_ws_floats
    for args in ((0, 1, 8, [4]), (-5, 1, 8, [4]), (1 << 31, 1, 8, [4]), (21, 0, 8, [4]), (21, 5, 8, [4] * 5), (21, 1, 0, [4]),
                 (21, 1, 1025, [4]), (21, 1, 8, [0]), (21, 2, 8, [4, 513])):
        assert f(args[0], args[1], args[2], _ints(args[3])) == 0, args
    Ts = [1, 21, 63, 64, 65, 260, 1024, 20480, 100000, 3_000_000, (1 << 31) - 1]
    for K0, N in ((1, [1]), (48, [96, 64]), (65, [100, 33, 64]), (1024, [512, 512, 512, 512])):
        got = [f(T, len(N), K0, _ints(N)) for T in Ts]
        assert got == [f(T, len(N), K0, _ints(N)) for T in Ts] and got == sorted(got), (K0, N, got)
        part = sum(n * (k + 1) for n, k in zip(N, [K0] + N[:-1]))
        assert got[0] >= sum(N) + part                                       # the rows dz_i and one split of partials
        assert got[-1] >= ((1 << 31) - 1) * sum(N)


# ---------------------------------------------------------------------------------------------------------- bounds and faults
# the shapes of tests/test_mlp_block_gpu.py
STACKS = [(1, [1], True, True, 0.3), (3, [33], False, False, 0.3), (48, [96, 64], True, True, 0.0), (48, [96, 64], False, True, 0.3),
          (65, [100, 33, 64], True, False, 0.3), (336, [128], False, True, 0.0), (1024, [512, 1, 512, 4], True, True, 0.3)]


def test_the_restated_masks_are_the_oracles():
    import device_rng

    keeps = R.keep_masks(SEED, OFFSET, 33, [100, 64], 0.3)
    for i, N in enumerate((100, 64)):
        want = device_rng.dropout_keep(SEED, device_rng.dropout_ctr_hi(OFFSET, i, ops.SITE_MLP_BLOCK), 33 * N, 0.3)
        assert torch.equal(keeps[i].view(-1), torch.from_numpy(want).bool())
        assert 0.6 < float(keeps[i].float().mean()) < 0.8
    assert not torch.equal(keeps[0][:, :64], keeps[1])
    assert all(bool(k.all()) for k in R.keep_masks(SEED, OFFSET, 5, [7], 0.0))
    assert R.inv_keep(0.0) == 1.0 and abs(R.inv_keep(0.3) - 1 / 0.7) < 1e-7


@pytest.mark.parametrize("K0,dims,relu,bias,p", STACKS)
@pytest.mark.parametrize("T", [33, 260])
def test_the_fp32_torch_chain_stays_inside_the_bounds(T, K0, dims, relu, bias, p):
    k = R.make_case(T, K0, dims, bias)
    keeps = R.keep_masks(SEED, OFFSET, T, dims, p)
    acts, grads = R.torch_chain(k, relu, p, keeps)
    bs = k["bs"] if bias else None
    for i, (want, bound) in enumerate(R.forward(k["x"], k["Ws"], bs, relu, p, keeps, acts=acts)):
        assert R.ratio(acts[i], want, bound) <= 1.0, ("a", i)
    ref = R.backward(k["dout"], k["x"], k["Ws"], bs, acts, relu, p, keeps, k["dW0"], k["db0"])
    assert R.ratio(grads["dx"], *ref["dx"]) <= 1.0
    for i in range(len(dims)):
        assert R.ratio(grads["dW"][i], *ref["dW"][i]) <= 1.0, ("dW", i)
        if bias:
            assert R.ratio(grads["db"][i], *ref["db"][i]) <= 1.0, ("db", i)


@pytest.mark.parametrize("T,K0,dims", [(33, 3, [33]), (129, 48, [96, 64]), (260, 65, [100, 33, 64]), (127, 1024, [512, 1, 512, 4])])
def test_planted_faults_exceed_their_bounds(T, K0, dims):
    """each planted fault of the restatement lies far outside the bounds at the GPU test's shapes (ReLU, bias, p = 0.3)"""
    relu, p, n = True, 0.3, len(dims)
    k = R.make_case(T, K0, dims, True)
    keeps = R.keep_masks(SEED, OFFSET, T, dims, p)
    good = R.forward(k["x"], k["Ws"], k["bs"], relu, p, keeps)
    acts = [a.float() for a, _ in good]

    def worst_forward(fault, masks=keeps):
        bad = R.forward(k["x"], k["Ws"], k["bs"], relu, p, masks, fault=fault, acts=acts)
        ok = R.forward(k["x"], k["Ws"], k["bs"], relu, p, keeps, acts=acts)
        return max(R.ratio(b[0].float(), *g) for b, g in zip(bad, ok))

    assert worst_forward("no_bias") > 10.0
    assert worst_forward("no_scale") > 10.0
    assert worst_forward("last_act_skipped") > 10.0
    assert worst_forward(None, R.keep_masks(SEED, OFFSET, T, dims, p, fault="mask_transposed")) > 10.0
    if n > 1:       # layer 0 has no previous layer: its counter is its own
        prev = R.keep_masks(SEED, OFFSET, T, dims, p, fault="mask_prev_layer")
        assert worst_forward(None, [keeps[0]] + prev[1:]) > 10.0
    ref = R.backward(k["dout"], k["x"], k["Ws"], k["bs"], acts, relu, p, keeps, k["dW0"], k["db0"])
    bad = R.backward(k["dout"], k["x"], k["Ws"], k["bs"], acts, relu, p, keeps, k["dW0"], k["db0"], fault="gate_from_z")
    assert R.ratio(bad["dx"][0].float(), *ref["dx"]) > 10.0
    assert max(R.ratio(bad["dW"][i][0].float(), *ref["dW"][i]) for i in range(n)) > 10.0
    bad = R.backward(k["dout"], k["x"], k["Ws"], k["bs"], acts, relu, p, keeps, k["dW0"], k["db0"], fault="db_overwritten")
    assert min(R.ratio(bad["db"][i][0].float(), *ref["db"][i]) for i in range(n)) > 10.0
    assert set(R.FAULTS) == {"no_bias", "no_scale", "mask_transposed", "mask_prev_layer", "gate_from_z", "db_overwritten",
                             "last_act_skipped"}


# ---------------------------------------------------------------------------------------------------------- operators
def test_operators_are_registered_and_their_fakes_give_the_shapes():
    assert {"mlp_stack", "mlp_stack_bwd"} <= set(torch_ops.OPERATORS)
    for name in ("mlp_stack", "mlp_stack_bwd"):
        assert str(getattr(torch.ops.t4r_hip, name).default._schema).startswith(f"t4r_hip::{name}(")
    m = lambda *s: torch.empty(*s, device="meta")     # noqa: E731
    assert torch.ops.t4r_hip.mlp_stack(m(5, 7, 48), [m(96, 48), m(64, 96)], [m(96), m(64)], True, 0.1, 1, 2).shape == (5, 7, 64)
    assert torch.ops.t4r_hip.mlp_stack(m(35, 48), [m(64, 48)], [], False, 0.0, 0, 0).shape == (35, 64)
    g = torch.ops.t4r_hip.mlp_stack_bwd(m(5, 7, 64), m(5, 7, 48), [m(96, 48), m(64, 96)], [m(96), m(64)], True, 0.1, 1, 2)
    assert [tuple(t.shape) for t in g] == [(5, 7, 48), (96, 48), (64, 96), (96,), (64,)]
    g = torch.ops.t4r_hip.mlp_stack_bwd(m(35, 64), m(35, 48), [m(64, 48)], [], False, 0.0, 0, 0)
    assert [tuple(t.shape) for t in g] == [(35, 48), (64, 48)]


def test_make_fx_traces_the_operator_and_its_backward_on_meta_tensors():
    def f(x, W0, W1, b0, b1):
        out = torch.ops.t4r_hip.mlp_stack(x, [W0, W1], [b0, b1], True, 0.1, 1, 2)
        return torch.autograd.grad(out.sum(), (x, W0, W1, b0, b1))

    m = lambda *s: torch.empty(*s, device="meta", requires_grad=True)     # noqa: E731
    gm = make_fx(f, tracing_mode="fake")(m(5, 7, 48), m(96, 48), m(64, 96), m(96), m(64))
    targets = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
    assert "t4r_hip.mlp_stack.default" in targets and "t4r_hip.mlp_stack_bwd.default" in targets, targets


# ---------------------------------------------------------------------------------------------------------- module
def test_constructor_refusals():
    for kw, word in ((dict(activation=torch.nn.GELU), "activation"), (dict(activation=torch.nn.Tanh), "activation"),
                     (dict(normalization="batch_norm"), "normalization"), (dict(filter_features=["a"]), "filter_features")):
        with pytest.raises(NotImplementedError, match=word):
            MLPBlock([64], **kw)
    for shape, dims in (([-1, 20, 1025], [64]), ([-1, 20, 48], [513]), ([-1, 20, 48], [8, 8, 8, 8, 8]), ([-1, 20, 48], [])):
        with pytest.raises(NotImplementedError, match="fused stack"):
            MLPBlock(dims).build(torch.Size(shape))
    with pytest.raises(ValueError, match="dropout"):
        MLPBlock([8], dropout=1.0).build([-1, 20, 48])
    assert tr.MLPBlock is MLPBlock and tr.block.MLPBlock is MLPBlock
    assert MLPBlock(64).dimensions == [64]


def test_built_module_names_initialisation_and_sizes():
    torch.manual_seed(3)
    stack = MLPBlock([96, 64], dropout=0.1).build(torch.Size([-1, 20, 48]))
    assert isinstance(stack, MLPStack) and stack._t4r_hip and isinstance(stack[0], DenseBlock)
    assert {k: tuple(v.shape) for k, v in stack.state_dict().items()} == {"0.0.weight": (96, 48), "0.0.bias": (96,),
                                                                         "1.0.weight": (64, 96), "1.0.bias": (64,)}
    assert stack.forward_output_size(torch.Size([8, 20, 48])) == torch.Size([8, 20, 64])
    assert stack.output_size() == torch.Size([-1, 20, 64]) and stack[0].forward_output_size([8, 20, 48]) == torch.Size([8, 20, 96])
    assert (stack.in_features, stack.out_features, stack.relu, stack.use_bias, stack.dropout) == (48, 64, True, True, 0.1)
    assert stack._get_name() == "SequentialBlock" and stack[0]._get_name() == "DenseBlock"
    # exactly torch.nn.Linear's initialisation: the same draws from the same generator state
    torch.manual_seed(3)
    for i, (k, n) in enumerate(((48, 96), (96, 64))):
        lin = torch.nn.Linear(k, n)
        assert torch.equal(stack[i][0].weight, lin.weight) and torch.equal(stack[i][0].bias, lin.bias)
    assert {id(p) for p in tr.hip_parameters(stack)} == {id(p) for p in stack.parameters()}
    assert stack._drop_offset == 0 and isinstance(stack.seed, int)
    state = tr.get_rng_state(stack)
    assert state[""]["_drop_offset"] == 0 and state[""]["_seed"] == stack.seed
    state[""]["_drop_offset"] = 5
    tr.set_rng_state(stack, state)
    assert stack._drop_offset == 5
    plain = MLPBlock([64], activation=None, use_bias=False).build([-1, 20, 48])
    assert list(plain.state_dict()) == ["0.0.weight"] and not plain.relu and not plain.use_bias and plain.dropout == 0.0
    with pytest.raises(_lib.T4RHipError, match="GPU"):
        stack(torch.zeros(2, 20, 48))


def _parts(d_item=48, d_model=64, masking="clm"):
    torch.manual_seed(0)
    feats = tr.TabularSequenceFeatures.from_schema(tr.session_schema(V, L), max_sequence_length=L, masking=masking,
                                                   aggregation="concat", embedding_dims={"item_id": d_item})
    cfg = tr.XLNetConfig.build(d_model=d_model, n_head=4, n_layer=2, total_seq_length=L, dropout=0.0)
    return feats, tr.TransformerBlock(cfg, masking=feats.masking)


def _keys(model):
    return {k: tuple(v.shape) for k, v in model.state_dict().items()}


def test_model_with_the_block_has_the_three_entry_body():
    from transformers4rec_amd.model import last_rows_gate

    feats, block = _parts()
    model = tr.Model(feats, block, tr.NextItemPredictionTask(weight_tying=True), mlp_block=MLPBlock([96, 64], dropout=0.1))
    body = model.heads[0].body
    assert len(body) == 3 and body[0] is feats and body[2] is block and isinstance(body[1], MLPStack)
    assert model.input_features is feats and model.transformer_block is block and model.mlp_block is body[1]
    keys = _keys(model)
    assert keys["heads.0.body.1.0.0.weight"] == (96, 48) and keys["heads.0.body.1.1.0.bias"] == (64,)
    assert keys["heads.0.body.0._masking.masked_item_embedding"] == (48,)             # the input block keeps its own width
    assert keys["heads.0.body.2.transformer.layer.0.rel_attn.q"] == (64, 4, 16)
    assert keys["heads.0.prediction_task_dict.next-item.task_block.0.0.weight"] == (48, 64)   # the task sees the transformer's width
    assert not any(k.startswith("heads.0.body.1.transformer") for k in keys)
    assert "heads.0.body.1" in tr.get_rng_state(model)
    assert {id(p) for p in body[1].parameters()} <= {id(p) for p in tr.hip_parameters(model)}
    # the last-rows path stays available to a three-entry body: the gate decides on the same grounds
    mlm = tr.Model(*_parts(masking="mlm"), tr.NextItemPredictionTask(weight_tying=True), mlp_block=MLPBlock([64])).train()
    two = tr.Model(*_parts(64, masking="mlm"), tr.NextItemPredictionTask(weight_tying=True)).train()
    assert last_rows_gate(mlm, True, 8, L, n_labels=3) == last_rows_gate(two, True, 8, L, n_labels=3)
    # a built stack is taken as it is; widths that do not fit are refused
    feats, block = _parts()
    built = MLPBlock([64]).build(feats.output_size())
    assert tr.Model(feats, block, tr.NextItemPredictionTask(weight_tying=True), mlp_block=built).mlp_block is built
    for bad in (MLPBlock([96]), MLPBlock([64]).build([-1, L, 32])):
        with pytest.raises(ValueError, match="mlp_block maps"):
            tr.Model(*_parts(), tr.NextItemPredictionTask(weight_tying=True), mlp_block=bad)
    with pytest.raises(TypeError, match="mlp_block"):
        tr.Model(*_parts(), tr.NextItemPredictionTask(weight_tying=True), mlp_block=torch.nn.Linear(48, 64))


def test_out_of_scope_uses_raise():
    feats, block = _parts()
    with pytest.raises(NotImplementedError):
        tr.TabularSequenceFeatures.from_schema(tr.session_schema(V, L), max_sequence_length=L, masking="clm", aggregation="concat",
                                               projection=MLPBlock([64]))
    ctx = tr.SequenceEmbeddingFeatures({"category": (13, 24)}, aggregation="concat")
    with pytest.raises(NotImplementedError, match="post_context_module"):
        tr.Model(feats, block, tr.NextItemPredictionTask(weight_tying=True), mlp_block=MLPBlock([64]), post_context_module=ctx)
    model = tr.Model(*_parts(masking="mlm"), tr.NextItemPredictionTask(weight_tying=True), mlp_block=MLPBlock([64]))
    from transformers4rec_amd import functional
    with pytest.raises(NotImplementedError, match="mlp_block"):
        functional.config_of(model)


def test_a_model_without_the_block_keeps_its_state_dict_keys():
    """the key list of the parent commit, from a committed fixture of a two-entry body (its p/* entries are one name per tensor:
    every one must be a key, and every key must be one of them or share its tensor with one)"""
    import golden_utils as gu

    d = gu.load("xlnet_clm_item_train")
    ref = {k: tuple(v.shape) for k, v in gu.section(d, "p/").items()}
    Lf, Vf, Df = int(d["meta/L"]), int(d["meta/V"]), int(d["meta/d_model"])
    feats = tr.TabularSequenceFeatures.from_schema(tr.session_schema(Vf - 1, Lf), max_sequence_length=Lf, masking="clm",
                                                   aggregation="concat", embedding_dims={"item_id": Df})
    cfg = tr.XLNetConfig.build(d_model=Df, n_head=int(d["meta/n_head"]), n_layer=int(d["meta/n_layer"]), total_seq_length=Lf, dropout=0.0)
    tied = not any(k.endswith("output_layer") for k in ref)              # as the fixture's reference model was built
    model = tr.Model(feats, tr.TransformerBlock(cfg, masking=feats.masking), tr.NextItemPredictionTask(weight_tying=tied))
    own = _keys(model)
    assert ref and all(own.get(k) == v for k, v in ref.items()), [k for k, v in ref.items() if own.get(k) != v]
    assert model.mlp_block is None and len(model.heads[0].body) == 2
    assert all(k.startswith(("heads.0.body.0.", "heads.0.body.1.", "heads.0.prediction_task_dict.next-item.")) for k in own)
    assert not any(k.startswith("heads.0.body.2") for k in own)
    by_ptr = {v.data_ptr() for k, v in model.state_dict().items() if k in ref}
    assert all(v.data_ptr() in by_ptr for v in model.state_dict().values())          # no tensor the parent did not have


# ---------------------------------------------------------------------------------------------------------- reference, fixtures
def _reference():
    import ref_standins as rs

    if not os.path.isdir(rs.REFERENCE_ROOT):
        pytest.skip("the reference tree is not on this machine")
    return rs.import_reference()


FIXTURES = {"mlp_body_clm_train": dict(dimensions=[96, 64]),
            "mlp_body_linear_clm_train": dict(dimensions=[64], activation=None, use_bias=False)}


def _mirror(d):
    dims = [int(v) for v in str(d["meta/dimensions"]).split(",")]
    feats = tr.TabularSequenceFeatures.from_schema(tr.session_schema(int(d["meta/V"]) - 1, int(d["meta/L"])),
                                                   max_sequence_length=int(d["meta/L"]), masking="clm", aggregation="concat",
                                                   embedding_dims={"item_id": int(d["meta/d_item"])})
    cfg = tr.XLNetConfig.build(d_model=int(d["meta/d_model"]), n_head=int(d["meta/n_head"]), n_layer=int(d["meta/n_layer"]),
                               total_seq_length=int(d["meta/L"]), dropout=0.0)
    mlp = MLPBlock(dims, activation=torch.nn.ReLU if int(d["meta/relu"]) else None, use_bias=bool(int(d["meta/use_bias"])))
    return tr.Model(feats, tr.TransformerBlock(cfg, masking=feats.masking), tr.NextItemPredictionTask(weight_tying=True), mlp_block=mlp)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_state_dict_names_and_shapes_equal_the_references(name):
    import sys

    ref_tr = _reference()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_mlp_block_golden as tool
    finally:
        sys.path.pop(0)
    ref = {k: tuple(v.shape) for k, v in tool.build_reference(ref_tr, name).state_dict().items()}
    import golden_utils as gu

    own = _keys(_mirror(gu.load(name)))
    stack = {k: v for k, v in ref.items() if k.startswith("heads.0.body.1.")}
    assert stack and all(own.get(k) == v for k, v in stack.items()), stack
    assert {k for k in own if k.startswith("heads.0.body.1.")} == set(stack)
    assert ref["heads.0.body.0._masking.masked_item_embedding"] == own["heads.0.body.0._masking.masked_item_embedding"] == (48,)
    moved = {k: v for k, v in ref.items() if k.startswith("heads.0.body.2.")}
    assert moved and all(own.get(k) == v for k, v in moved.items() if "inv_freq" not in k and "position_ids" not in k)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixture_parameters_have_a_home_in_the_mirror_and_hold_data_only(name):
    import golden_utils as gu

    d = gu.load(name)
    assert os.path.getsize(os.path.join(gu.GOLDEN, name + ".npz")) <= 900 * 1024
    assert all(v.dtype.kind in "fiubU" for v in d.values())                 # arrays of numbers and meta strings, nothing else
    own = _keys(_mirror(d))
    ref = {k: tuple(v.shape) for k, v in gu.section(d, "p/").items()}
    assert ref and all(own.get(k) == v for k, v in ref.items()), [k for k, v in ref.items() if own.get(k) != v]
    assert "heads.0.body.1.0.0.weight" in ref and ("heads.0.body.1.0.0.bias" in ref) == bool(int(d["meta/use_bias"]))
    grads = gu.section(d, "g/")
    assert len(grads) >= 20 and "heads.0.body.1.0.0.weight" in grads and "heads.0.body.0._masking.masked_item_embedding" in grads
    assert tuple(d["out/mlp"].shape) == (8, 20, 64) and tuple(d["out/hidden"].shape) == (8, 20, 64)
