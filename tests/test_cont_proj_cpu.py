"""Host half of `continuous_projection`: the ninth C-ABI header (include/t4r_hip_contproj.h) against the library, the size
query and the argument limits (refused before any launch), the module mirror's construction, state-dict names against the
reference classes built live (oracle/ref_standins.py), the refusals, the drop-in conversion and the documents.  Nothing here
needs a GPU."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

import transformers4rec_amd as tr
from transformers4rec_amd import _lib, features as F, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTS = ("price", "age_days", "hour")
SORTED = ["age_days", "hour", "price"]
FOUR = ["t4r_cont_proj_bwd", "t4r_cont_proj_bwd_ws_floats", "t4r_cont_proj_fwd", "t4r_cont_proj_supported"]


# ---------------------------------------------------------------------------------------------------------- header and ABI
def test_contproj_header_library_and_prototypes_agree():
    lib = _lib.load()
    syms = _lib.header_symbols("t4r_hip_contproj.h")
    assert syms == FOUR
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/t4r_hip_contproj.h but not exported"
    text = open(_lib.header_path("t4r_hip_contproj.h")).read()
    for entry in ("int t4r_cont_proj_fwd(void* stream", "int t4r_cont_proj_bwd(void* stream"):
        decl = text[: text.index(entry)]
        comment = decl[decl.rindex("/*"):]
        assert "replaces:" in comment and "block/mlp.py" in comment, entry
    decls = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for word in ("at::", "torch", "Tensor", "std::", "c10"):
        assert word not in decls, f"{word} leaked into the C ABI"


def test_ws_floats_is_pure_and_monotone():
    f = _lib.load().t4r_cont_proj_bwd_ws_floats
    assert f(0, 3, 24) == 0 and f(-5, 3, 24) == 0
    assert f(100, 0, 24) == 0 and f(100, 65, 24) == 0 and f(100, 3, 0) == 0 and f(100, 3, 1025) == 0
    Ts = [1, 63, 64, 65, 129, 1280, 16383, 16384, 16385, 20480, 100000, 3_000_000]
    for C, P in ((1, 1), (3, 24), (16, 100), (64, 1024)):
        got = [f(T, C, P) for T in Ts]
        assert got == [f(T, C, P) for T in Ts] and got == sorted(got) and got[0] >= P * (C + 1), (C, P, got)
    for T in (1, 300, 20480):
        got = [f(T, 8, P) for P in (1, 4, 6, 64, 65, 100, 128, 129, 1024)]
        assert got == sorted(got) and got[0] > 0, got


def _fwd(lib, C, P, T=4, L=1):
    buf = ctypes.c_void_p(1 << 20)        # never dereferenced: every failing case below is refused before any launch
    return lib.t4r_cont_proj_fwd(None, buf, buf, T, L, C, P, buf, buf, buf)


def _bwd(lib, C, P, T=4, L=1, ld=None, col=0):
    buf = ctypes.c_void_p(1 << 20)
    return lib.t4r_cont_proj_bwd(None, buf, P if ld is None else ld, col, buf, buf, T, L, C, P, buf, buf, buf, buf, None, buf)


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_argument_limits_are_refused_before_any_launch(call):
    lib = _lib.load()
    for kw, word in ((dict(C=0, P=8), b"C <= 64"), (dict(C=65, P=8), b"C <= 64"), (dict(C=3, P=0), b"P <= 1024"),
                     (dict(C=3, P=1025), b"P <= 1024"), (dict(C=3, P=8, T=-1), b"ntok"), (dict(C=3, P=8, T=10, L=3), b"divide")):
        rc = call(lib, **kw)
        assert rc != 0, kw
        assert word in lib.t4r_last_error(), (kw, lib.t4r_last_error())
    assert call(lib, C=3, P=8, T=0) == 0                                   # nothing to do: nothing launches
    assert lib.t4r_cont_proj_fwd(None, None, None, 0, 1, 3, 8, None, None, None) == 0
    assert lib.t4r_cont_proj_supported(1, 1) == 1 and lib.t4r_cont_proj_supported(64, 1024) == 1
    assert [lib.t4r_cont_proj_supported(*a) for a in ((0, 8), (65, 8), (3, 0), (3, 1025))] == [0, 0, 0, 0]


def test_backward_refuses_a_short_pitch_and_null_pointers():
    lib = _lib.load()
    assert _bwd(lib, 3, 8, ld=7) != 0 and b"ld below col + P" in lib.t4r_last_error()
    assert _bwd(lib, 3, 8, ld=10, col=3) != 0 and b"ld below col + P" in lib.t4r_last_error()
    assert lib.t4r_cont_proj_fwd(None, None, None, 4, 1, 3, 8, None, None, None) != 0 and b"null" in lib.t4r_last_error()


def test_ops_wrappers_check_their_arguments():
    xs = [torch.zeros(2, 5), torch.zeros(2)]
    W, b = torch.zeros(8, 2), torch.zeros(8)
    with pytest.raises(_lib.T4RHipError):
        ops.cont_proj_fwd(xs, [False, True], W, b)
    with pytest.raises(_lib.T4RHipError):
        ops.cont_proj_bwd_(torch.zeros(10, 8), 0, xs, [False, True], W, b, torch.zeros(8, 2), torch.zeros(8))
    with pytest.raises(ValueError):
        ops.cont_proj_fwd(xs, [False], W, b)
    with pytest.raises(ValueError):
        ops.cont_proj_fwd([], [], W, b)


# ---------------------------------------------------------------------------------------------------------- host construction
def _schema(conts=CONTS, L=10, V=50):
    return tr.session_schema(V, L, (("category", 7),), conts)


def _block(dims, **kw):
    args = dict(max_sequence_length=10, masking="mlm", d_output=32, embedding_dims={"item_id": 16, "category": 8},
                continuous_projection=dims)
    args.update(kw)
    return tr.TabularSequenceFeatures.from_schema(_schema(), **args)


@pytest.mark.parametrize("dims,want", [(24, [24]), ([12, 20], [12, 20])])
def test_from_schema_builds_the_projected_module(dims, want):
    f = _block(dims)
    cont = f.continuous_module
    assert isinstance(cont, F.ContinuousProjection) and cont.dims == want and cont.names == SORTED
    assert isinstance(cont[0], F.ContinuousFeatures) and list(cont[0].parameters()) == [] and list(cont[2].parameters()) == []
    assert f._feature_order == ["category", "continuous_projection", "item_id"]
    assert not set(CONTS) & set(f._feature_order) and not set(CONTS) & set(f._dims)
    assert f._dims["continuous_projection"] == want[-1]
    assert f._cols == {"category": 0, "continuous_projection": 8, "item_id": 8 + want[-1]} and f._agg_width == 24 + want[-1]
    assert f.output_size() == torch.Size([-1, 10, 32])
    assert f.projection_module[0][0].weight.shape == (32, 24 + want[-1])
    sizes = [3] + want
    keys = {}
    for i, (a, b) in enumerate(zip(sizes[:-1], sizes[1:])):
        keys[f"to_merge.continuous_module.1.{i}.0.weight"] = (b, a)
        keys[f"to_merge.continuous_module.1.{i}.0.bias"] = (b,)
    got = {k: tuple(v.shape) for k, v in f.state_dict().items() if "continuous_module" in k}
    assert got == keys
    plain = tr.TabularSequenceFeatures.from_schema(_schema(), max_sequence_length=10, aggregation="concat",
                                                   embedding_dims={"item_id": 16, "category": 8})
    assert plain.output_size()[-1] == 27 and _block(dims, d_output=None, masking=None).output_size()[-1] == 24 + want[-1]


def test_linear_default_init():
    torch.manual_seed(0)
    lin = _block(64).continuous_module.layers[0].requires_grad_(False)
    bound = 1 / 3 ** 0.5          # kaiming_uniform(a = sqrt 5) on fan-in 3, and the bias
    assert float(lin.weight.abs().max()) <= bound and float(lin.bias.abs().max()) <= bound
    assert float(lin.weight.abs().max()) > 0.8 * bound and float(lin.weight.std()) > 0.2


def test_project_continuous_features_on_a_built_block():
    f = tr.TabularSequenceFeatures.from_schema(_schema(), max_sequence_length=10, aggregation="concat", d_output=32,
                                               embedding_dims={"item_id": 16, "category": 8})
    assert isinstance(f.continuous_module, F.ContinuousFeatures) and f._agg_width == 27
    assert f.project_continuous_features([12, 20]) is f
    g = _block([12, 20], masking=None)
    assert {k: tuple(v.shape) for k, v in f.state_dict().items()} == {k: tuple(v.shape) for k, v in g.state_dict().items()}
    assert f._feature_order == g._feature_order and f._cols == g._cols and f._agg_width == g._agg_width == 44
    assert repr(f.continuous_module) == repr(g.continuous_module)
    with pytest.raises(ValueError, match="projected already"):
        f.project_continuous_features(8)
    bare = tr.TabularSequenceFeatures.from_schema(tr.session_schema(50, 10), max_sequence_length=10)
    with pytest.raises(ValueError, match="continuous"):
        bare.project_continuous_features(8)


def test_element_wise_widths():
    kw = dict(aggregation="element-wise-sum", embedding_dims={"item_id": 16, "category": 16})
    f = _block([12, 16], **kw)
    assert f._agg_width == 16 and f._cols == {"category": 0, "continuous_projection": 0, "item_id": 0}
    with pytest.raises(ValueError, match="same dimension"):
        _block([12, 20], **kw)


def test_refusals_name_the_argument():
    with pytest.raises(NotImplementedError, match="post.*continuous_projection"):
        _block(24, post="layer-norm")
    with pytest.raises(NotImplementedError, match="continuous_soft_embeddings"):
        _block(24, continuous_soft_embeddings=True)
    with pytest.raises(ValueError, match="continuous_projection.*no continuous column"):
        tr.TabularSequenceFeatures.from_schema(tr.session_schema(50, 10), max_sequence_length=10, continuous_projection=24)
    with pytest.raises(NotImplementedError, match="projection"):
        tr.TabularSequenceFeatures.from_schema(_schema(), max_sequence_length=10, projection=torch.nn.Linear(3, 3))
    with pytest.raises(NotImplementedError, match="continuous_projection"):
        _block(2048)                                           # the first layer's width limit
    with pytest.raises(ValueError):
        _block([])
    # `pre` stays: the swap noise acts on the raw columns
    f = _block(24, pre="stochastic-swap-noise")
    assert f.continuous_module._pre is not None and f.continuous_module._pre is f.continuous_module[0]._pre
    # the registered-operator path refuses
    from transformers4rec_amd import functional

    model = type("M", (), {"input_features": _block(24)})()
    with pytest.raises(NotImplementedError, match="continuous_projection"):
        functional.input_block_of(model)


def test_new_parameters_are_ordinary_dense_parameters():
    f = _block([12, 20])
    dense, tables = tr.flatten_model(f)
    names = [n for n, _p, _o in dense.entries]
    for i in (0, 1):
        for w in ("weight", "bias"):
            assert f"to_merge.continuous_module.1.{i}.0.{w}" in names
    assert not any("continuous_module" in n for n, _p, _o in tables.entries)
    carried = {id(p) for p in tr.hip_parameters(f)}
    assert all(id(p) in carried for p in f.continuous_module.parameters())


# ------------------------------------------------------------------------------------------------ against the reference, live
def _reference():
    import ref_standins as rs

    if not os.path.isdir(rs.REFERENCE_ROOT):
        pytest.skip("the reference tree is not on this machine")
    spec = importlib.util.spec_from_file_location("make_contproj_golden", os.path.join(ROOT, "tools", "make_contproj_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return rs.import_reference(), mod


def _mirror(mod, name):
    c = mod.CASES[name]
    schema = tr.session_schema(mod.V, mod.L, mod.CATS, mod.CONTS)
    return tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=mod.L, masking="mlm", aggregation=c["aggregation"],
                                                  d_output=mod.D_MODEL, embedding_dims={"item_id": c["d_item"], "category": c["d_cat"]},
                                                  continuous_projection=c["dims"])


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


@pytest.mark.parametrize("name", ["xlnet_mlm_contproj_train", "xlnet_mlm_contproj2_train"])
def test_state_dict_keys_equal_the_reference_classes(name):
    ref_tr, mod = _reference()
    ref = mod.build_reference(ref_tr, name).heads[0].body[0]
    ours = _mirror(mod, name)
    assert _shapes(ours.continuous_module) == _shapes(ref.to_merge["continuous_module"])
    assert _shapes(ours) == _shapes(ref)
    n = len(mod.CASES[name]["dims"]) if isinstance(mod.CASES[name]["dims"], list) else 1
    assert sum("continuous_module" in k for k in _shapes(ours)) == 2 * n


def test_dropin_converts_and_shares_the_mlp():
    ref_tr, mod = _reference()
    from transformers4rec_amd import dropin

    for name in mod.CASES:
        model = mod.build_reference(ref_tr, name)
        keys = list(model.state_dict().keys())
        dropin.convert_model(model, ref_tr)
        ref = model.heads[0].body[0]
        sh = ref.hip_shadow()
        assert list(model.state_dict().keys()) == keys
        assert isinstance(sh.continuous_module, F.ContinuousProjection) and sh.continuous_module.names == SORTED
        assert sh._feature_order == ["category", "continuous_projection", "item_id"]
        ref_params = dict(ref.named_parameters())
        n = 0
        for pname, p in sh.named_parameters():
            assert p is ref_params[pname] and p.device.type != "meta", pname
            n += "continuous_module" in pname
        assert n == 2 * len(sh.continuous_module.dims)
        assert sh.continuous_module.layers[0].weight is ref.to_merge["continuous_module"][1][0][0].weight
    assert "continuous_projection" not in dropin.__doc__.split("Configurations off the hot path")[1].split("raise NotImplementedError")[0]


def test_dropin_refuses_other_mlps_and_other_first_members():
    ref_tr, mod = _reference()
    from transformers4rec.torch.block.base import SequentialBlock
    from transformers4rec.torch.block.mlp import MLPBlock
    from transformers4rec.torch.tabular.base import AsTabular
    from transformers4rec_amd import dropin

    def rebuilt(**mlp_kw):
        ref = mod.build_reference(ref_tr, "xlnet_mlm_contproj_train").heads[0].body[0]
        cont = ref.to_merge["continuous_module"][0]
        ref.to_merge["continuous_module"] = SequentialBlock(cont, MLPBlock([24], **mlp_kw), AsTabular("continuous_projection"))
        return ref

    with pytest.raises(NotImplementedError, match="dropout"):
        dropin.shadow_features(rebuilt(dropout=0.1))
    with pytest.raises(NotImplementedError, match="normalization"):
        dropin.shadow_features(rebuilt(normalization="batch_norm"))
    with pytest.raises(NotImplementedError, match="activation"):
        dropin.shadow_features(rebuilt(activation=torch.nn.ELU))
    with pytest.raises(NotImplementedError, match="bias"):
        dropin.shadow_features(rebuilt(use_bias=False))
    ref = mod.build_reference(ref_tr, "xlnet_mlm_contproj_train").heads[0].body[0]
    seq = ref.to_merge["continuous_module"]
    ref.to_merge["continuous_module"] = SequentialBlock(SequentialBlock(seq[0]), seq[1], seq[2])
    with pytest.raises(NotImplementedError, match="ContinuousFeatures"):
        dropin.shadow_features(ref)


# ---------------------------------------------------------------------------------------------------------- documents
def test_documents_name_the_new_surface():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "t4r_hip_contproj.h" in readme and re.search(r"\b4 continuous-projection entry points", readme)
    assert "cont_proj.hip" in readme
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in FOUR + ["t4r_hip_contproj.h", "continuous_module.1.<i>.0.weight", "continuous_projection"]:
        assert word in integ, word
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 4.9" in design and "cont_proj.hip" in design and "T·(4C + 4P)" in design
    assert "cont_proj.hip" in open(os.path.join(ROOT, "transformers4rec_amd", "build.py")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "cont_proj_bench.py"))
